// ddc_host.cpp -- the down-converter's per-sample arithmetic (basebandboard_amd/csrc/ddc_common.hpp: the mixer step and the
// CORDIC) run on the CPU.  Built by tests/test_ddc_host.py with -fsanitize=address,undefined and run as a program.
//
// usage: ddc_host walk STRIDE
//   walks the (I, Q) pairs of int16 x int16 -- every I, and for each I the Q values -32768 + (I mod STRIDE) + m STRIDE, so
//   STRIDE 1 is all 2^32 pairs -- plus every pair of the corner values, with the CORDIC on int64 accumulators beside the int32
//   one: the two must agree, max(|X|, |Y|) must stay below 2^31 and mag at or below 65535.  Prints the largest |X|, |Y| and mag.
// usage: ddc_host vectors FILE
//   FILE holds int32 values: npairs, then npairs times (i, q, mag, phase); then pa0, fcw, first, n, the 1024 ROM entries, and
//   n times (x, mi, mq), where sample k has the absolute number first + k.  Every value must be reproduced.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../basebandboard_amd/csrc/ddc_common.hpp"

using namespace bbb;

namespace {

long long g_xmax = 0;
unsigned g_magmax = 0;

bool pair_ok(int i, int q) {
    uint32_t m64, m32;
    int p64, p32;
    int64_t top = 0;
    ddc_polar_t<int64_t>(i, q, m64, p64, &top);
    if (top >= (1ll << 31) || m64 > 65535u) {
        std::fprintf(stderr, "pair (%d, %d): max |X|,|Y| = %lld, mag = %u\n", i, q, (long long)top, m64);
        return false;
    }
    ddc_polar(i, q, m32, p32);
    if (m32 != m64 || p32 != p64) {
        std::fprintf(stderr, "pair (%d, %d): int32 (%u, %d) != int64 (%u, %d)\n", i, q, m32, p32, m64, p64);
        return false;
    }
    if (top > g_xmax) g_xmax = top;
    if (m64 > g_magmax) g_magmax = m64;
    return true;
}

int walk(long long stride) {
    if (stride < 1) return 2;
    const int corner[] = {-32768, -32767, -1, 0, 1, 32767};
    for (int i : corner)
        for (int q : corner)
            if (!pair_ok(i, q)) return 1;
    unsigned long long pairs = 0;
    for (int i = -32768; i <= 32767; ++i)
        for (long long q = -32768 + (i + 32768) % stride; q <= 32767; q += stride, ++pairs)
            if (!pair_ok(i, (int)q)) return 1;
    std::printf("pairs %llu max_xy %lld max_mag %u\n", pairs, g_xmax, g_magmax);
    return 0;
}

int vectors(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<int32_t> v((size_t)bytes / 4);                       // exactly the file: a read beyond it is found
    if (std::fread(v.data(), 4, v.size(), f) != v.size()) return 2;
    std::fclose(f);
    size_t at = 0;
    const int npairs = v.at(at++);
    for (int k = 0; k < npairs; ++k, at += 4) {
        uint32_t m;
        int p;
        ddc_polar(v.at(at), v.at(at + 1), m, p);
        if ((int)m != v.at(at + 2) || p != v.at(at + 3)) {
            std::fprintf(stderr, "cordic (%d, %d): got (%u, %d), want (%d, %d)\n", v[at], v[at + 1], m, p, v[at + 2], v[at + 3]);
            return 1;
        }
    }
    const uint32_t pa0 = (uint32_t)v.at(at), fcw = (uint32_t)v.at(at + 1), first = (uint32_t)v.at(at + 2);
    const int n = v.at(at + 3);
    at += 4;
    std::vector<int16_t> rom(1024);
    for (int k = 0; k < 1024; ++k) rom[k] = (int16_t)v.at(at++);
    for (int k = 0; k < n; ++k, at += 3) {
        const uint32_t adr = ddc_adr(pa0, fcw, first + (uint32_t)k);
        int mi, mq;
        ddc_mix(v.at(at), rom.at((adr + 256u) & 1023u), rom.at(adr), mi, mq);
        if (mi != v.at(at + 1) || mq != v.at(at + 2)) {
            std::fprintf(stderr, "mixer sample %d (x = %d): got (%d, %d), want (%d, %d)\n", k, v[at], mi, mq, v[at + 1], v[at + 2]);
            return 1;
        }
    }
    if (at != v.size()) return 2;
    std::printf("pairs %d samples %d\n", npairs, n);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "walk")) return walk(std::atoll(argv[2]));
    if (argc == 3 && !std::strcmp(argv[1], "vectors")) return vectors(argv[2]);
    std::fprintf(stderr, "usage: ddc_host walk STRIDE | ddc_host vectors FILE\n");
    return 2;
}
