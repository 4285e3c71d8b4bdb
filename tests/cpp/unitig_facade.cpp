// C++ consumer of s2k::Engine::graph_unitigs and s2k::Engine::graph_unitig_edges (tests/test_unitigs.py builds and links it; on a GPU
// it runs: both calls refused for a missing CSR; prints "unitigs ok refused N M").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        int refused_unitigs = 0, refused_edges = 0;
        try {
            s2k_unitig_out out{};
            uint64_t n_links = 0;
            (void)eng.graph_unitigs(nullptr, nullptr, 0, 1, &out, &n_links);
        } catch (const s2k::Error &e) {
            refused_unitigs = (int)e.status;
        }
        try {
            (void)eng.graph_unitig_edges(nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0);
        } catch (const s2k::Error &e) {
            refused_edges = (int)e.status;
        }
        std::printf("unitigs ok refused %d %d\n", refused_unitigs, refused_edges);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
