// C++ consumer of s2k::Table::vote_keys / vote_representatives and s2k::Engine::vote_ordinals (tests/test_vote.py builds and links
// it; on a GPU it runs: the calls refuse a batch description without its arrays, and the ordinals of no nodes are no work; prints
// "vote ok refused A B C").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        s2k::Table table(eng, nullptr, nullptr, 0), votes(eng, nullptr, nullptr, 0);
        int refused_keys = 0, refused_best = 0, refused_ord = 0;
        s2k_device_out in{};
        try {
            (void)table.vote_keys(0, in, 3, nullptr, nullptr);
        } catch (const s2k::Error &e) {
            refused_keys = (int)e.status;
        }
        try {
            table.vote_representatives(votes, 0, in, 3, nullptr, nullptr, 0, nullptr);
        } catch (const s2k::Error &e) {
            refused_best = (int)e.status;
        }
        try {
            eng.vote_ordinals(nullptr, 0, nullptr);
        } catch (const s2k::Error &e) {
            refused_ord = (int)e.status;
        }
        std::printf("vote ok refused %d %d %d\n", refused_keys, refused_best, refused_ord);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
