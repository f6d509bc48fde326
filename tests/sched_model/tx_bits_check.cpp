// The data bits of a chunk against the buffer its object allocates for them: for each of the four bit-range functions of
// bbb_common.hpp (eye, sweep, link, xcorr) and every chunk size 1..4096 (and the default 2^26 and the largest, 2^30), the bits that
// any chunk of up to that size needs -- at first samples that straddle bit 0 and the sample-17 / sample-45 origins, and far
// from them -- fit the words that *_bits_words gives the open.  tx_chunks.hpp's tx_chunk_bits refuses a range that does not
// fit at run time ("internal: ..."); this says that it never has to.  Host arithmetic only: nothing of HIP is called.
#include <cstdio>
#include <vector>

#include "bbb_common.hpp"

using namespace bbb;

static long long g_checked = 0;

// what tx_chunk_bits does with a range: clamp at bit 0, count
static void fits(const char *who, BitRange r, uint64_t words, uint64_t chunk, uint64_t first, uint64_t n) {
    const int64_t lo = std::max<int64_t>(0, r.lo);
    const uint64_t nbits = r.hi >= lo ? (uint64_t)(r.hi - lo + 1) : 0;
    g_checked++;
    if (nbits > words * 64) {
        std::printf("%s: chunk %llu first %llu n %llu needs %llu bits, the buffer holds %llu\n", who, (unsigned long long)chunk,
                    (unsigned long long)first, (unsigned long long)n, (unsigned long long)nbits, (unsigned long long)(words * 64));
        std::exit(1);
    }
}

int main() {
    std::vector<uint64_t> firsts;
    for (uint64_t f = 0; f <= 72; f++) firsts.push_back(f);                      // bit 0, sample 17 (+ 8 m), sample 45 (+ 8 m)
    for (uint64_t base : {1ull << 20, 1ull << 40, (1ull << 62) - (1ull << 31)})
        for (uint64_t d = 0; d < 16; d++) firsts.push_back(base - 8 + d);
    std::vector<uint64_t> chunks;
    for (uint64_t c = 1; c <= 4096; c++) chunks.push_back(c);
    chunks.push_back(1ull << 26);
    chunks.push_back(1ull << 30);
    const uint32_t delays[] = {0, 1, 7, 8, 9, 255}, groups[] = {1, 2, 5, 32}, lags[] = {1, 2, 8, 9, 64, 65, 511, 512};
    for (uint64_t chunk : chunks)
        for (uint64_t first : firsts)
            for (uint64_t n : {chunk, (uint64_t)1, chunk / 2 + 1}) {                // a whole chunk, and ragged last ones
                fits("eye", eye_bit_range(first, n), eye_bits_words(chunk), chunk, first, n);
                fits("sweep", sweep_bit_range(first, n), sweep_bits_words(chunk), chunk, first, n);
                for (uint32_t delay : delays)
                    for (uint32_t ng : groups) {
                        // (bbb_link_sweep_run: the outputs re-timed by the delay, the first tile aligned to the noise's origin)
                        const int64_t lead = 8 * (int64_t)ng, out_lo = (int64_t)first + delay, norg = std::max<int64_t>(0, out_lo - lead);
                        const int64_t tb = out_lo - ((out_lo - norg) & 7);
                        fits("link", link_bit_range(tb, lead, out_lo + (int64_t)n), link_bits_words(chunk) - 1, chunk, first, n);
                    }
                for (uint32_t nl : lags)
                    fits("xcorr", xcorr_bit_range(first, n, bbb_xcorr_cfg{8, nl, BBB_TX_BIT_ORIGIN}), xcorr_bits_words(chunk, nl), chunk, first, n);
            }
    std::printf("ok %lld ranges\n", g_checked);
    return 0;
}
