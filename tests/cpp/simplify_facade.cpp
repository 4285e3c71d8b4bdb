// C++ consumer of s2k::Engine::graph_simplify_mask and s2k::Engine::graph_induced (tests/test_simplify.py builds and links it; on a
// GPU it runs: both calls refused for missing arrays; prints "simplify ok refused N M").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        int refused_mask = 0, refused_induced = 0;
        try {
            (void)eng.graph_simplify_mask(nullptr, nullptr, 0, 1, nullptr, nullptr, 4, 8, nullptr);
        } catch (const s2k::Error &e) {
            refused_mask = (int)e.status;
        }
        try {
            (void)eng.graph_induced(nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr,
                                    nullptr, 0);
        } catch (const s2k::Error &e) {
            refused_induced = (int)e.status;
        }
        std::printf("simplify ok refused %d %d\n", refused_mask, refused_induced);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
