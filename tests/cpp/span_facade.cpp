// C++ consumer of s2k::Engine::paths_spans and s2k::Engine::graph_resolve_mask (tests/test_span.py builds and links it; on a GPU it
// runs: no unitigs, no steps and no spans are accepted, spans without a path_off array refused; prints "span ok refused N").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        const s2k::Engine::ResolveTotals r = eng.graph_resolve_mask(nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 2, nullptr, nullptr);
        s2k_thread_out paths{};
        int refused = 0;
        try {
            (void)eng.paths_spans(0, paths, 0, nullptr, nullptr, 0, nullptr, 0);
        } catch (const s2k::Error &e) {
            refused = (int)e.status;
        }
        std::printf("span ok refused %d resolved %llu\n", refused, (unsigned long long)r.resolved);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
