// C++ consumer of s2k::Counter and the Engine's merge / counting file mode (tests/test_count_merge.py builds and links it; on a GPU it
// runs: argv[1] = a FASTA/FASTQ file, argv[2] = min_count; prints "distinct N solid M kminmers K").
#include "s2k.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    try {
        s2k::Engine eng(0);
        s2k::Counter counter(eng);
        s2k_params p{31, 7, 0.01, S2K_MODE_HPC, 0};
        s2k_counts tot = eng.run_file_count(argv[1], p, 1u << 20, counter.raw());
        s2k::Engine::CountSizes r = counter.finish((uint32_t)std::strtoul(argv[2], nullptr, 10));
        s2k::Engine::CountSizes e = eng.count_merge(nullptr, nullptr, 0, nullptr, nullptr, 0, 1);
        counter.add(nullptr, 0);
        std::printf("distinct %llu solid %llu kminmers %llu empty %llu\n", (unsigned long long)r.n_distinct, (unsigned long long)r.n_kept,
                    (unsigned long long)tot.n_kminmers, (unsigned long long)e.n_distinct);
    } catch (const s2k::Error &e) {
        std::fprintf(stderr, "s2k error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
