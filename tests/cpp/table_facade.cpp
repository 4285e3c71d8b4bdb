// C++ consumer of s2k::Table (tests/test_count_table.py builds and links it; on a GPU it runs: an empty table, a look-up of nothing,
// a filter refused for a missing input; prints "table ok refused N").
#include "s2k.hpp"

#include <cstdio>

int main() {
    try {
        s2k::Engine eng(0);
        s2k::Table table(eng, nullptr, nullptr, 0);
        table.lookup(nullptr, 0, nullptr);
        int refused = 0;
        try {
            s2k_device_out in{};
            s2k_solid_out out{};
            (void)table.filter(1, in, 2, out); // in.km_off == nullptr
        } catch (const s2k::Error &e) {
            refused = (int)e.status;
        }
        std::printf("table ok refused %d\n", refused);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
