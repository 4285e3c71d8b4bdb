// C++ consumer of s2k::Table::edges and s2k::Engine::graph_adjacency (tests/test_graph.py builds and links it; on a GPU it runs: an
// empty table, edges refused for a missing rev array, an adjacency refused for a missing row_off array; prints
// "graph ok refused N M").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        s2k::Table table(eng, nullptr, nullptr, 0);
        int refused_edges = 0, refused_adj = 0;
        try {
            s2k_device_out in{}; // in.km_off == in.hash == in.rev == nullptr
            (void)table.edges(1, in, 2);
        } catch (const s2k::Error &e) {
            refused_edges = (int)e.status;
        }
        try {
            eng.graph_adjacency(nullptr, 0, 1, nullptr);
        } catch (const s2k::Error &e) {
            refused_adj = (int)e.status;
        }
        std::printf("graph ok refused %d %d\n", refused_edges, refused_adj);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
