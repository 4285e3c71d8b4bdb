// C++ consumer of s2k::Table::representatives / node_sequences and s2k::Engine::unitig_sequences (tests/test_unitig_sequences.py
// builds and links it; on a GPU it runs: an empty table accepts an empty batch description only with its arrays, and the stitch
// refuses a missing uni_off; prints "seq ok refused A B C").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        s2k::Table table(eng, nullptr, nullptr, 0);
        int refused_rep = 0, refused_nodes = 0, refused_stitch = 0;
        s2k_device_out in{};
        try {
            table.representatives(0, in, 0, nullptr);
        } catch (const s2k::Error &e) {
            refused_rep = (int)e.status;
        }
        try {
            (void)table.node_sequences(0, in, 3, nullptr, nullptr, 0, nullptr);
        } catch (const s2k::Error &e) {
            refused_nodes = (int)e.status;
        }
        try {
            s2k_node_seqs nodes{};
            (void)eng.unitig_sequences(nullptr, nullptr, nullptr, 0, 0, nodes, nullptr);
        } catch (const s2k::Error &e) {
            refused_stitch = (int)e.status;
        }
        std::printf("seq ok refused %d %d %d\n", refused_rep, refused_nodes, refused_stitch);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
