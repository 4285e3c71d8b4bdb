// compiles and links the walk wrappers of include/s2k.hpp (tests/test_walk.py); run without a GPU it only reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        s2k_node_seqs nodes{};
        s2k_thread_out paths{};
        s2k_unitig_out lift{};
        s2k_walk_out out{};
        const uint64_t n = eng.unitig_member_offsets(nullptr, nullptr, nullptr, 0, 0, nodes, nullptr);
        const s2k::Engine::WalkTotals t = eng.paths_walks(0, paths, 0, nullptr, nullptr, 0, lift, 0, nullptr, nullptr, nullptr, nullptr, &out);
        std::printf("%llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)t.walks, (unsigned long long)t.followed,
                    (unsigned long long)t.off_graph);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
