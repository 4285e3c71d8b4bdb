// compiles and links the segmented-alignment wrappers of include/s2k.hpp (tests/test_align_segments.py); run without a GPU it only
// reports that there is none
#include <cstdio>

#include "s2k.hpp"

int main() {
    try {
        s2k::Engine eng(0);
        const uint64_t off[2] = {0, 0};
        s2k_walk_out walks{};
        walks.walk_off = const_cast<uint64_t *>(off);
        s2k_thread_out paths{}, src{};
        src.path_off = const_cast<uint64_t *>(off);
        s2k_device_out in{};
        in.km_off = const_cast<uint64_t *>(off);
        const s2k::Engine::SegmentLift lift{nullptr, nullptr, nullptr, 0, nullptr, off, nullptr, nullptr, 0};
        const s2k::Engine::SegmentSource source{&src, 0, nullptr, nullptr, &in};
        const s2k::Engine::Segments sg = eng.walks_segments(0, walks, 0, paths, 0, lift, nullptr, off, nullptr, source);
        s2k_align_out seg{}, out{};
        seg.ops_off = const_cast<uint64_t *>(off);
        const uint64_t m = eng.align_join(0, off, nullptr, 0, seg, &out);
        std::printf("%llu %llu %llu\n", (unsigned long long)sg.n_segments, (unsigned long long)sg.stats[0], (unsigned long long)m);
    } catch (const s2k::Error &e) {
        std::printf("no engine: %s\n", e.what());
    }
    return 0;
}
