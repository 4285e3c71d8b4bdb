// compiles and links the bridge wrapper of include/s2k.hpp (tests/test_bridge.py); run without a GPU it only reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        s2k_thread_out paths{}, out{};
        const s2k::Engine::BridgeTotals t = eng.paths_bridge(0, paths, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 16, 2, out);
        std::printf("%llu %llu %llu\n", (unsigned long long)t.steps, (unsigned long long)t.merged, (unsigned long long)t.bridged);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
