// xcorr_host.cpp -- the per-lane core of the correlation kernel (basebandboard_amd/csrc/xcorr_common.hpp) run on the CPU, lane
// by lane, in the kernel's geometry: tiles cut at the 16-byte boundary of the sample pointer, 256 lanes per workgroup, gx
// workgroups striding over the tiles, one grid row per XT lag groups, int64 lag arrays folded at the end.  Built by
// tests/test_xcorr_host.py with -fsanitize=address,undefined and compared there with tests/xcorr_model.py.
//
// usage: xcorr_host CASES OUT.  CASES holds cases back to back, each ten int64 values (spb, nlags, origin, first_sample,
// bit0, nbits, nsamples, a, gx, 0) followed by the samples (int16, padded to a multiple of 4) and the packed bit
// words (ceil(nbits / 64) u64).  `a` plays the pointer's offset from a 16-byte boundary in samples.  OUT receives one line of
// nlags counters per case.  Samples and bits live in heap blocks of exactly their size, so a read beyond either is found.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../basebandboard_amd/csrc/xcorr_common.hpp"

using namespace bbb;

namespace {

struct Case {
    long long spb, nlags, origin, first, bit0, nbits, nsamples, a, gx, reserved;
    std::vector<int16_t> x;
    std::vector<unsigned long long> bits;
};

template <int XT>
void run_rows(const Case &c, unsigned spb_sh, unsigned gy, std::vector<long long> &xc) {
    const long long ubase = c.first - c.origin - c.a;
    const long long ntiles = (c.nsamples + c.a + kXcorrTile - 1) / kXcorrTile;
    const long long nwords = (c.nbits + 63) / 64;
    const unsigned spb = 1u << spb_sh, lw = (unsigned)XT << spb_sh;
    const unsigned seg_sh = 5 + spb_sh;
    std::vector<int16_t> S((kXcorrSteps + 1) * kXcorrThreads);
    for (unsigned y = 0; y < gy; y++) {
        const unsigned jbase = y * XT;
        for (long long bx = 0; bx < c.gx && bx < ntiles; bx++) {
            std::vector<unsigned long long> Lg(lw, 0);
            std::vector<XcorrLane<XT>> lanes(kXcorrThreads);
            std::vector<char> masked(kXcorrThreads, 1);
            for (auto &l : lanes) l.clear();
            for (long long t = bx; t < ntiles; t += c.gx) {
                const long long ub = ubase + t * kXcorrTile, ib = t * kXcorrTile - c.a;
                if (ub + kXcorrTile <= 0) continue;
                for (auto &v : S) v = 0x7777;                         // the unused halfwords: never read
                for (unsigned k = 0; k < (unsigned)kXcorrTile; k++) {
                    const long long i = ib + k;
                    int16_t v = (i >= 0 && i < c.nsamples) ? c.x[(size_t)i] : (int16_t)0;
                    if (ub + k < 0) v = 0;
                    S[xcorr_lds_index(k, spb_sh)] = v;
                }
                for (unsigned tid = 0; tid < (unsigned)kXcorrThreads; tid++) {
                    const unsigned cc = tid & (spb - 1), s = tid >> spb_sh;
                    const unsigned r = xcorr_floor_mod(ubase + cc, spb_sh);
                    auto sink = [&](int j, long long v) {
                        const unsigned lag = ((jbase + (unsigned)j) << spb_sh) + r;
                        if (lag < (unsigned)c.nlags) Lg[((unsigned)j << spb_sh) + r] += (unsigned long long)v;
                    };
                    const long long q0 = xcorr_floor_div(ub + cc + ((long long)s << seg_sh), spb_sh);
                    bool m = masked[tid] != 0;
                    xcorr_lane_tile<XT>(lanes[tid], m, q0, jbase, c.bits.data(), c.bit0, nwords,
                                        [&](int step) { return (int)S[xcorr_lds_index(xcorr_lane_sample(tid, (unsigned)step, spb_sh), spb_sh)]; },
                                        sink);
                    masked[tid] = m;
                }
            }
            for (unsigned tid = 0; tid < (unsigned)kXcorrThreads; tid++) {
                const unsigned cc = tid & (spb - 1);
                const unsigned r = xcorr_floor_mod(ubase + cc, spb_sh);
                auto sink = [&](int j, long long v) {
                    const unsigned lag = ((jbase + (unsigned)j) << spb_sh) + r;
                    if (lag < (unsigned)c.nlags) Lg[((unsigned)j << spb_sh) + r] += (unsigned long long)v;
                };
                xcorr_flush(lanes[tid], masked[tid] != 0, sink);
            }
            for (unsigned i = 0; i < lw; i++) {
                const unsigned lag = y * lw + i;
                if (lag < (unsigned)c.nlags) xc[lag] = (long long)((unsigned long long)xc[lag] + Lg[i]);
            }
        }
    }
}

bool read_case(FILE *f, Case &c) {
    long long h[10];
    if (fread(h, sizeof(long long), 10, f) != 10) return false;
    c.spb = h[0], c.nlags = h[1], c.origin = h[2], c.first = h[3], c.bit0 = h[4], c.nbits = h[5], c.nsamples = h[6];
    c.a = h[7], c.gx = h[8], c.reserved = h[9];
    const size_t padded = ((size_t)c.nsamples + 3) / 4 * 4, nwords = ((size_t)c.nbits + 63) / 64;
    std::vector<int16_t> raw(padded);
    if (padded && fread(raw.data(), 2, padded, f) != padded) return false;
    c.x.assign(raw.begin(), raw.begin() + c.nsamples);
    c.x.shrink_to_fit();
    c.bits.assign(nwords, 0);
    c.bits.shrink_to_fit();
    if (nwords && fread(c.bits.data(), 8, nwords, f) != nwords) return false;
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    Case c;
    int ncases = 0;
    while (read_case(in, c)) {
        unsigned sh = 0;
        while ((1ll << sh) < c.spb) sh++;
        const unsigned J = (unsigned)((c.nlags + c.spb - 1) / c.spb);
        const int xt = J <= 8 ? 8 : J <= 16 ? 16 : 32;
        const unsigned gy = (J + xt - 1) / xt;
        std::vector<long long> xc((size_t)c.nlags, 0);
        if (xt == 8) run_rows<8>(c, sh, gy, xc);
        else if (xt == 16) run_rows<16>(c, sh, gy, xc);
        else run_rows<32>(c, sh, gy, xc);
        for (long long l = 0; l < c.nlags; l++) fprintf(out, "%lld%c", xc[(size_t)l], l + 1 == c.nlags ? '\n' : ' ');
        ncases++;
    }
    fclose(in);
    fclose(out);
    printf("cases %d\n", ncases);
    return 0;
}
