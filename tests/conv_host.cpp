// conv_host.cpp -- the kernel's walk of bbb_conv_decode restated on the CPU around the SAME per-lane core
// (basebandboard_amd/csrc/conv_common.hpp): workgroups of wpg windows that stage their span of steps depunctured through the
// period's table, waves of 64 lanes with one state per lane, the predecessors' metrics fetched by lane number, the survivor word
// made of the 64 lanes' bits, the butterfly for the end state, the traceback in the window's lane 0 and the packed output ORed
// word by word; and the encoder's walk, one output word at a time.  Built with -fsanitize=address,undefined by
// tests/test_conv_host.py, which compares the output with tests/conv_model.py.
//
//   conv_host cases.bin out.txt
// cases.bin: per case 24 int64 (mode, nvals, nbefore, K, n, gen[0..2], init_state, period, keep[0..2], terminated, B, W, D,
// first_step, final, threads, wpg, hard, in_off, 0) and nvals int16 (padded to a multiple of 4).  mode 0, decode: the values are
// the history and the call's received values (bits 0 / 1 with hard), placed in_off elements / bits behind the buffer's base;
// out.txt gets a line "ndecided windows" and a line of the packed words in hex.  mode 1, encode: the values are the nvals input
// bits, `nbefore` holds the state word; out.txt gets a line "nout state" and a line of the packed words.
#include "../basebandboard_amd/csrc/conv_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace bbb;

namespace {

constexpr int kWave = 64;
constexpr int16_t kPoison = 0x7ABC;                // a staged value no window may depend on

struct Case {
    int64_t mode, nvals, nbefore, K, n, gen[3], init, period, keep[3], terminated, B, W, D, first, final, threads, wpg, hard, in_off, pad;
};

template <typename T>
T shfl(const T (&v)[kWave], int src) { return v[src]; }

template <int N>
void decode(const Case &c, const std::vector<int16_t> &vals, std::vector<uint64_t> &bits, uint64_t &ndecided, uint64_t &windows) {
    MlseGeom geom;
    ConvPunct P;
    uint32_t gen[3], keep[3];
    for (int i = 0; i < 3; ++i) gen[i] = (uint32_t)c.gen[i], keep[i] = (uint32_t)c.keep[i];
    if (!conv_geom((uint32_t)c.B, (uint32_t)c.W, (uint32_t)c.D, geom) || !conv_punct((uint32_t)c.n, (uint32_t)c.period, keep, P)) std::abort();
    const int K = (int)c.K, NS = 1 << (K - 1);
    const bool hard = c.hard != 0;
    // the buffer as the caller lays it out: exactly the elements that exist, so that a read outside them is caught
    const uint64_t in_first = (uint64_t)(c.in_off + c.nbefore), nin = (uint64_t)(c.nvals - c.nbefore);
    std::vector<int16_t> soft;
    std::vector<uint64_t> packed;
    const void *in;
    if (hard) {
        packed.assign((size_t)(c.in_off + c.nvals + 63) / 64, 0);
        for (int64_t i = 0; i < c.nvals; ++i) packed[(size_t)(c.in_off + i) >> 6] |= (uint64_t)(vals[(size_t)i] & 1) << ((c.in_off + i) & 63);
        in = packed.data();
    } else {
        soft.assign((size_t)c.in_off, kPoison);
        soft.insert(soft.end(), vals.begin(), vals.begin() + c.nvals);
        in = soft.data();
    }
    const uint64_t first = (uint64_t)c.first, nsteps = conv_steps_below(P, conv_idx(P, first) + nin) - first;
    ndecided = mlse_ndecided(geom, first, nsteps, c.final != 0);
    bits.assign((ndecided + 63) / 64, 0);
    windows = 0;
    if (!ndecided) return;
    const uint64_t wanted = conv_idx(P, first) - conv_idx(P, mlse_window(geom, first / geom.B, first, 0, 0).a_lo);
    const int64_t rel_lo = -(int64_t)((uint64_t)c.nbefore < wanted ? (uint64_t)c.nbefore : wanted);
    const int64_t rel_hi = (int64_t)(conv_idx(P, first + nsteps) - conv_idx(P, first));
    const uint32_t B = geom.B, W = geom.W, D = geom.D, WL = B + W + D, nthr = (uint32_t)c.threads, wpg = (uint32_t)c.wpg;
    const uint32_t init = (uint32_t)c.init & (uint32_t)(NS - 1);
    const bool forced_end = c.terminated && c.final;
    const uint64_t j0 = first / B, nblocks = (first + ndecided - 1) / B - j0 + 1, end = first + nsteps;
    const uint64_t ngrp = (nblocks + wpg - 1) / wpg, idx_first = conv_idx(P, first);
    for (uint64_t grp = 0; grp < ngrp; ++grp) {
        const uint64_t jg = j0 + grp * wpg;
        const uint32_t nwin = (uint32_t)(wpg < j0 + nblocks - jg ? wpg : j0 + nblocks - jg);
        // the stage, as the kernel lays it out: step T at index T - lo_u, N values a step
        std::vector<int16_t> stage(((size_t)wpg * B + W + D) * N, kPoison);
        const int64_t lo_u = (int64_t)(jg * B) - (int64_t)W;
        const uint64_t T_lo = lo_u > 0 ? (uint64_t)lo_u : 0, T_hi = end < (jg + nwin) * B + D ? end : (jg + nwin) * B + D;
        const uint32_t r0 = (uint32_t)(T_lo % P.p);
        const int64_t base = (int64_t)conv_idx(P, T_lo) - (int64_t)idx_first;
        for (uint32_t i = 0; i < (uint32_t)(T_hi - T_lo); ++i) {
            uint32_t r;
            const int64_t rel = conv_value_of_step(P, base, r0, i, r);
            if (r != (T_lo + i) % P.p || rel != (int64_t)conv_idx(P, T_lo + i) - (int64_t)idx_first) std::abort();   // the table against the division
            int16_t v[kConvMaxN];
            conv_step_values(P, in, hard, in_first, rel, rel_lo, rel_hi, r, v);
            for (int k = 0; k < N; ++k) stage.at(((size_t)((int64_t)T_lo - lo_u) + i) * N + k) = v[k];
        }
        for (uint32_t w = 0; w < nthr / kWave; ++w) {
            std::vector<uint64_t> surv(WL);
            int32_t m[kWave];
            ConvLane rule[kWave];
            MlseWindow win[kWave];
            bool valid[kWave];
            int src0[kWave], src1[kWave];
            uint32_t wi[kWave], s_lo[kWave], s_hi[kWave];
            for (int lane = 0; lane < kWave; ++lane) {
                const uint32_t h = (uint32_t)lane & (uint32_t)(NS - 1), gbase = (uint32_t)lane & ~(uint32_t)(NS - 1);
                rule[lane] = conv_lane(gen, N, K, h);
                src0[lane] = (int)(gbase | conv_pred(h, 0, K));
                src1[lane] = (int)(gbase | conv_pred(h, 1, K));
                wi[lane] = w * (kWave / NS) + (uint32_t)lane / NS;
                valid[lane] = wi[lane] < nwin;
                win[lane] = mlse_window(geom, jg + wi[lane], first, nsteps, ndecided);
                m[lane] = conv_start(win[lane].from_zero, h, init);
                s_lo[lane] = valid[lane] ? (uint32_t)((int64_t)win[lane].a_lo - win[lane].lo) : 0u;
                s_hi[lane] = valid[lane] ? (uint32_t)((int64_t)win[lane].a_hi - win[lane].lo) : 0u;
                if (s_hi[lane] > WL) std::abort();
            }
            for (uint32_t s = 0; s < WL; ++s) {
                int32_t mn[kWave];
                uint64_t word = 0;
                for (int lane = 0; lane < kWave; ++lane) {
                    const bool active = s >= s_lo[lane] && s < s_hi[lane];
                    int16_t v[N];
                    for (int k = 0; k < N; ++k) v[k] = stage.at(((size_t)(valid[lane] ? wi[lane] : 0) * B + s) * N + k);
                    uint32_t ch;
                    const int32_t x = conv_acs<N>(rule[lane], v, shfl(m, src0[lane]), shfl(m, src1[lane]), ch);
                    mn[lane] = active ? x : m[lane];
                    word |= (uint64_t)ch << lane;
                }
                for (int lane = 0; lane < kWave; ++lane) m[lane] = mn[lane];
                surv[s] = word;
            }
            uint32_t best[kWave];
            for (int lane = 0; lane < kWave; ++lane) best[lane] = (uint32_t)lane & (uint32_t)(NS - 1);
            for (int d = 1; d < NS; d <<= 1) {
                int32_t nm[kWave];
                uint32_t nb[kWave];
                for (int lane = 0; lane < kWave; ++lane) {
                    const int32_t om = shfl(m, lane ^ d);
                    const uint32_t ob = shfl(best, lane ^ d);
                    const bool keep_own = conv_keeps(m[lane], best[lane], om, ob);
                    nm[lane] = keep_own ? m[lane] : om;
                    nb[lane] = keep_own ? best[lane] : ob;
                }
                for (int lane = 0; lane < kWave; ++lane) m[lane] = nm[lane], best[lane] = nb[lane];
            }
            for (int lane = 0; lane < kWave; lane += NS) {
                if (!valid[lane]) continue;
                ++windows;
                const MlseWindow &wn = win[lane];
                uint32_t s = forced_end && wn.a_hi == end ? 0u : best[lane];
                uint64_t out = 0;
                for (uint32_t i = WL; i-- > W;) {
                    const uint64_t T = (uint64_t)(wn.lo + (int64_t)i);
                    if (T >= wn.a_hi) continue;
                    if (T < wn.e_lo) break;
                    uint32_t bit;
                    s = conv_back(surv.at(i), (uint32_t)lane, s, K, bit);
                    if (T < wn.e_hi) {
                        const uint64_t k = T - first;
                        out |= (uint64_t)bit << (k & 63);
                        if ((k & 63) == 0 || T == wn.e_lo) {
                            bits.at(k >> 6) |= out;
                            out = 0;
                        }
                    }
                }
            }
        }
    }
}

void encode(const Case &c, const std::vector<int16_t> &vals, std::vector<uint64_t> &out, uint64_t &nout, uint32_t &state) {
    ConvPunct P;
    uint32_t gen[3], keep[3];
    for (int i = 0; i < 3; ++i) gen[i] = (uint32_t)c.gen[i], keep[i] = (uint32_t)c.keep[i];
    if (!conv_punct((uint32_t)c.n, (uint32_t)c.period, keep, P)) std::abort();
    const uint64_t first = (uint64_t)c.first, nsteps = (uint64_t)c.nvals, idx_first = conv_idx(P, first);
    std::vector<uint64_t> bits((size_t)(nsteps + 63) / 64, 0);
    for (uint64_t i = 0; i < nsteps; ++i) bits[(size_t)(i >> 6)] |= (uint64_t)(vals[(size_t)i] & 1) << (i & 63);
    state = (uint32_t)c.nbefore;
    nout = conv_idx(P, first + nsteps) - idx_first;
    out.assign((size_t)(nout + 63) / 64, 0);
    for (uint64_t wd = 0; wd < out.size(); ++wd) {
        const uint64_t x = idx_first + wd * 64;
        uint64_t period = x / P.ptot;
        uint32_t place = (uint32_t)(x % P.ptot);
        const uint32_t nb = (uint32_t)(nout - wd * 64 < 64 ? nout - wd * 64 : 64);
        uint64_t word = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const int64_t k = (int64_t)(period * P.p + P.inv_step[place] - first);
            if (k < 0 || k >= (int64_t)nsteps) std::abort();
            word |= (uint64_t)conv_parity(conv_in_window(bits.data(), state, k, (int)c.K) & gen[P.inv_bit[place]]) << b;
            if (++place == P.ptot) place = 0, ++period;
        }
        out[(size_t)wd] = word;
    }
    if (nsteps) {
        uint32_t h = 0;
        for (uint32_t i = 0; i + 1 < (uint32_t)c.K; ++i) h |= conv_in_bit(bits.data(), state, (int64_t)nsteps - 1 - (int64_t)i) << i;
        state = h;
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
        std::vector<int16_t> vals((size_t)(c.nvals + 3) / 4 * 4);
        if (!vals.empty() && std::fread(vals.data(), 2, vals.size(), f) != vals.size()) return 3;
        std::vector<uint64_t> bits;
        uint64_t a = 0, b = 0;
        if (c.mode == 0) {
            if (c.n == 2) decode<2>(c, vals, bits, a, b);
            else decode<3>(c, vals, bits, a, b);
        } else {
            uint32_t state;
            encode(c, vals, bits, a, state);
            b = state;
        }
        std::fprintf(o, "%llu %llu\n", (unsigned long long)a, (unsigned long long)b);
        for (uint64_t wd : bits) std::fprintf(o, "%llx ", (unsigned long long)wd);
        std::fprintf(o, "\n");
        ++cases;
    }
    std::fclose(f);
    std::fclose(o);
    std::printf("cases %d\n", cases);
    return 0;
}
