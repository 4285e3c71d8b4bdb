// C++ consumer of s2k::Engine::graph_untangle and s2k::Engine::unitig_expand (tests/test_untangle.py builds and links it; on a GPU it
// runs: no unitigs and no copies are accepted, edges without unitigs refused; prints "untangle ok refused N copies 0 members 0").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        const s2k::Engine::UntangleTotals u = eng.graph_untangle(nullptr, nullptr, 0, 0, nullptr, nullptr);
        int refused = 0;
        try {
            (void)eng.graph_untangle(nullptr, nullptr, 1, 0, nullptr, nullptr);
        } catch (const s2k::Error &e) {
            refused = (int)e.status;
        }
        s2k_unitig_out none{};
        const uint64_t m = eng.unitig_expand(none, 0, nullptr, none, 0, none);
        std::printf("untangle ok refused %d copies %llu members %llu\n", refused, (unsigned long long)u.copies, (unsigned long long)m);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
