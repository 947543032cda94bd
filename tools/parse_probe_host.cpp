// tools/parse_probe.py, leg (d): the example's FASTA reader rule (fmindex-collection_amd/example/main.cpp, readFasta: byte by byte through a class table, a record per
// '>' line) timed on one core over a synthetic single-line FASTA of <reads> x <length> bases made in memory.  Prints "<bytes> <reads> <symbols> <seconds>".
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    size_t const reads = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000, length = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 101;
    std::string bytes;
    bytes.reserve(reads * (length + 12));
    uint64_t state = 88172645463325252ull;
    char name[16];
    for (size_t r = 0; r < reads; ++r) {
        std::snprintf(name, sizeof name, ">r%08zu\n", r % 100000000);
        bytes += name;
        for (size_t i = 0; i < length; ++i) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; bytes.push_back("ACGT"[state & 3]); }
        bytes.push_back('\n');
    }
    std::array<uint8_t, 256> classes;
    classes.fill(7);
    classes['\n'] = 6; classes['$'] = 0;
    for (int r = 0; r < 4; ++r) classes[static_cast<unsigned char>("ACGT"[r])] = classes[static_cast<unsigned char>("acgt"[r])] = static_cast<uint8_t>(r + 1);
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<uint8_t>> records;
    size_t const size = bytes.size();
    size_t at = 0, symbols = 0;
    while (at < size) {
        while (at < size && bytes[at] != '\n') ++at;
        ++at;
        if (at >= size) break;
        std::vector<uint8_t> ranks;
        for (; at + 1 < size && bytes[at] != '>'; ++at) {
            uint8_t const cls = classes[static_cast<unsigned char>(bytes[at])];
            if (cls < 6) ranks.push_back(cls);
            else if (cls == 7) ranks.push_back(1);
        }
        symbols += ranks.size();
        records.push_back(std::move(ranks));
        if (at + 1 >= size) break;
    }
    double const seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%zu %zu %zu %.6f\n", size, records.size(), symbols, seconds);
    return 0;
}
