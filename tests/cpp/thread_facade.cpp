// C++ consumer of s2k::Engine::unitig_node_places and s2k::Table::thread (tests/test_thread.py builds and links it; on a GPU it runs:
// an empty decomposition is accepted, threading without a path_off array refused; prints "thread ok refused N").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        eng.unitig_node_places(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr);
        s2k::Table table(eng, nullptr, nullptr, 0);
        s2k_device_out in{};
        s2k_thread_out out{};
        int refused = 0;
        try {
            (void)table.thread(0, in, 2, nullptr, 0, out, 0);
        } catch (const s2k::Error &e) {
            refused = (int)e.status;
        }
        std::printf("thread ok refused %d\n", refused);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
