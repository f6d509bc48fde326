// mlse_host.cpp -- the kernel's walk of bbb_mlse_run restated on the CPU around the SAME per-window core
// (basebandboard_amd/csrc/mlse_common.hpp): workgroups of threads / NS windows over a span of y values, waves of 64 lanes
// with one state per lane, the predecessors' metrics fetched by lane number, the survivor word made of the 64 lanes' bits,
// the butterfly for the end state, the traceback in the window's lane 0 and the packed output ORed word by word.  Built with
// -fsanitize=address,undefined by tests/test_mlse_host.py, which compares the output with tests/mlse_model.py.
//
//   mlse_host cases.bin out.txt
// cases.bin: per case 16 int64 (ny, -k_lo, mem, g[0..4], init_state, B, W, D, first_symbol, final, threads, 0) and ny int32
// y values (padded to an even count), y[i] the symbol k_lo + i counted from the call's first.  out.txt: per case a line
// "ndecided windows" and a line of the packed words in hex.
#include "../basebandboard_amd/csrc/mlse_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace bbb;

namespace {

constexpr int kWave = 64;
constexpr int16_t kPoison = 0x7ABC;                // a span value no window may depend on

struct Case {
    int64_t ny, nback, mem, g[5], init, B, W, D, first, final, threads, pad;
};

template <typename T>
T shfl(const T (&v)[kWave], int src) { return v[src]; }

void run(const Case &c, const std::vector<int32_t> &y, std::vector<uint64_t> &bits, uint64_t &ndecided, uint64_t &windows) {
    MlseGeom geom;
    if (!mlse_geom((uint32_t)c.B, (uint32_t)c.W, (uint32_t)c.D, geom)) std::abort();
    const int L = (int)c.mem, NS = 1 << L;
    int32_t g[kMlseMaxMem + 1];
    for (int i = 0; i <= kMlseMaxMem; ++i) g[i] = (int32_t)c.g[i];
    const uint64_t first = (uint64_t)c.first, nsym = (uint64_t)(c.ny - c.nback);
    ndecided = mlse_ndecided(geom, first, nsym, c.final != 0);
    bits.assign((ndecided + 63) / 64, 0);
    windows = 0;
    if (!ndecided) return;
    const uint32_t B = geom.B, W = geom.W, D = geom.D, WL = B + W + D, nthr = (uint32_t)c.threads, wpg = nthr / NS;
    const uint32_t init = (uint32_t)c.init & (uint32_t)(NS - 1);
    const uint64_t j0 = first / B, nblocks = (first + ndecided - 1) / B - j0 + 1, end = first + nsym;
    const uint64_t ngrp = (nblocks + wpg - 1) / wpg;
    for (uint64_t grp = 0; grp < ngrp; ++grp) {
        const uint64_t jg = j0 + grp * wpg;
        const uint32_t nwin = (uint32_t)(wpg < j0 + nblocks - jg ? wpg : j0 + nblocks - jg);
        // the span, as the kernel lays it out: index K - lo_u
        std::vector<int16_t> ys((size_t)wpg * B + W + D, kPoison);
        const int64_t lo_u = (int64_t)(jg * B) - (int64_t)W;
        const uint64_t K_lo = lo_u > 0 ? (uint64_t)lo_u : 0, K_hi = end < (jg + nwin) * B + D ? end : (jg + nwin) * B + D;
        for (uint64_t K = K_lo; K < K_hi; ++K) {
            const int64_t k = (int64_t)K - (int64_t)first;
            ys.at((size_t)((int64_t)K - lo_u)) = (int16_t)y.at((size_t)(k + c.nback));
        }
        for (uint32_t w = 0; w < nthr / kWave; ++w) {
            std::vector<uint64_t> surv(WL);
            int64_t m[kWave];
            MlseLane rule[kWave];
            MlseWindow win[kWave];
            bool valid[kWave];
            int src0[kWave], src1[kWave];
            uint32_t wi[kWave];
            for (int lane = 0; lane < kWave; ++lane) {
                const uint32_t h = (uint32_t)lane & (uint32_t)(NS - 1), gbase = (uint32_t)lane & ~(uint32_t)(NS - 1);
                rule[lane] = mlse_lane(g, L, h);
                src0[lane] = (int)(gbase | mlse_pred(h, 0, L));
                src1[lane] = (int)(gbase | mlse_pred(h, 1, L));
                wi[lane] = w * (kWave / NS) + (uint32_t)lane / NS;
                valid[lane] = wi[lane] < nwin;
                win[lane] = mlse_window(geom, jg + wi[lane], first, nsym, ndecided);
                m[lane] = mlse_start(win[lane].from_zero, h, init);
            }
            for (uint32_t s = 0; s < WL; ++s) {
                int64_t mn[kWave];
                uint64_t word = 0;
                for (int lane = 0; lane < kWave; ++lane) {
                    const int64_t K = win[lane].lo + (int64_t)s;
                    const bool active = valid[lane] && K >= (int64_t)win[lane].a_lo && K < (int64_t)win[lane].a_hi;
                    uint32_t ch;
                    const int64_t v = mlse_acs(rule[lane], ys.at((size_t)wi[lane] * B + s), shfl(m, src0[lane]), shfl(m, src1[lane]), ch);
                    mn[lane] = active ? v : m[lane];
                    word |= (uint64_t)ch << lane;
                }
                for (int lane = 0; lane < kWave; ++lane) m[lane] = mn[lane];
                surv[s] = word;
            }
            uint32_t best[kWave];
            for (int lane = 0; lane < kWave; ++lane) best[lane] = (uint32_t)lane & (uint32_t)(NS - 1);
            for (int d = 1; d < NS; d <<= 1) {
                int64_t nm[kWave];
                uint32_t nb[kWave];
                for (int lane = 0; lane < kWave; ++lane) {
                    const int64_t om = shfl(m, lane ^ d);
                    const uint32_t ob = shfl(best, lane ^ d);
                    const bool keep = mlse_keeps(m[lane], best[lane], om, ob);
                    nm[lane] = keep ? m[lane] : om;
                    nb[lane] = keep ? best[lane] : ob;
                }
                for (int lane = 0; lane < kWave; ++lane) m[lane] = nm[lane], best[lane] = nb[lane];
            }
            for (int lane = 0; lane < kWave; lane += NS) {
                if (!valid[lane]) continue;
                ++windows;
                const MlseWindow &wn = win[lane];
                uint32_t s = best[lane];
                uint64_t out = 0;
                for (uint32_t i = WL; i-- > W;) {
                    const uint64_t K = (uint64_t)(wn.lo + (int64_t)i);
                    if (K >= wn.a_hi) continue;
                    if (K < wn.e_lo) break;
                    uint32_t bit;
                    s = mlse_back(surv.at(i), (uint32_t)lane, s, L, bit);
                    if (K < wn.e_hi) {
                        const uint64_t k = K - first;
                        out |= (uint64_t)bit << (k & 63);
                        if ((k & 63) == 0 || K == wn.e_lo) {
                            bits.at(k >> 6) |= out;
                            out = 0;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    int cases = 0;
    Case c;
    while (std::fread(&c, sizeof c, 1, f) == 1) {
        std::vector<int32_t> y((size_t)(c.ny + 1) / 2 * 2);
        if (!y.empty() && std::fread(y.data(), 4, y.size(), f) != y.size()) return 3;
        std::vector<uint64_t> bits;
        uint64_t nd, windows;
        run(c, y, bits, nd, windows);
        std::fprintf(o, "%llu %llu\n", (unsigned long long)nd, (unsigned long long)windows);
        for (uint64_t wd : bits) std::fprintf(o, "%llx ", (unsigned long long)wd);
        std::fprintf(o, "\n");
        ++cases;
    }
    std::fclose(f);
    std::fclose(o);
    std::printf("cases %d\n", cases);
    return 0;
}
