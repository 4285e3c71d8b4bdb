// C++ consumer of s2k::Engine::graph_bubble_mask (tests/test_bubbles.py builds and links it; on a GPU it runs: refused for missing
// arrays and for max_nodes 0 and S2K_BUBBLE_MAX_NODES + 1; prints "bubble ok refused A B C").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        int refused[3] = {0, 0, 0};
        const uint32_t max_nodes[3] = {16, 0, S2K_BUBBLE_MAX_NODES + 1};
        for (int i = 0; i < 3; i++) {
            try {
                const s2k::Engine::BubbleTotals t = eng.graph_bubble_mask(nullptr, nullptr, 0, 1, nullptr, nullptr, max_nodes[i], 20, nullptr);
                (void)t.sources;
            } catch (const s2k::Error &e) {
                refused[i] = (int)e.status;
            }
        }
        std::printf("bubble ok refused %d %d %d\n", refused[0], refused[1], refused[2]);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
