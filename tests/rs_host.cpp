// rs_host.cpp -- the kernels' walk of bbb_rs_decode and bbb_rs_encode restated on the CPU around the SAME per-lane core
// (basebandboard_amd/csrc/rs_common.hpp): workgroups of four waves that stage four coded frames from their unaligned start
// (single bytes up to the first and behind the last 16-byte boundary, 16-byte pieces between), waves of 64 lanes with four
// symbols a lane, the syndromes packed four to a word and XORed over the lanes, Berlekamp-Massey with one coefficient a lane and
// the auxiliary polynomial moved up a lane per step, the roots counted over the lanes, the values in the lanes that found one,
// the correction in the stage, and the data stored as aligned words; and the encoder's walk, one codeword per lane.  Built with
// -fsanitize=address,undefined by tests/test_rs_host.py, which compares the output with tests/rs_model.py.
//
//   rs_host cases.bin out.txt
// cases.bin: per case 10 int64 (mode, prim_poly, fcr, prim, nroots, n, depth, nframes, in_off, out_off) and the input bytes
// (padded to a multiple of 8).  mode 0, decode: the bytes are nframes coded frames, placed in_off bytes behind an allocation's
// start, the data out_off bytes behind another's; out.txt gets a line with the five statistics, a line with nerr in hex and a
// line with the data in hex.  mode 1, encode: the bytes are nframes data frames; out.txt gets "0 0 0 0 0", an empty line and the
// coded bytes in hex.
#include "../basebandboard_amd/csrc/rs_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bbb;

namespace {

constexpr uint32_t kWave = 64, kWaves = 4, kThreads = kWave * kWaves, kFramesPerGroup = 4;
constexpr uint8_t kPoison = 0xA5;

struct Case {
    int64_t mode, prim_poly, fcr, prim, nroots, n, depth, nframes, in_off, out_off;
};

uint32_t wave_xor(const uint32_t (&v)[kWave]) {
    uint32_t r = 0;
    for (uint32_t l = 0; l < kWave; ++l) r ^= v[l];
    return r;
}

void decode(const RsField &F, const RsCode &c, const uint8_t *in, uint64_t nframes, uint8_t *out, uint8_t *nerr_out, uint64_t stats[5]) {
    const uint8_t *ex = F.ex, *lg = F.lg;
    const uint32_t I = c.depth, n = c.n, k = c.k, nroots = c.nroots, fbytes = I * n, dbytes = I * k;
    const uint64_t ngrp = (nframes + kFramesPerGroup - 1) / kFramesPerGroup;
    for (uint64_t grp = 0; grp < ngrp; ++grp) {
        const uint64_t f0 = grp * kFramesPerGroup;
        const uint32_t nfr = (uint32_t)(nframes - f0 < kFramesPerGroup ? nframes - f0 : kFramesPerGroup), bytes = nfr * fbytes;
        const uint8_t *src = in + f0 * fbytes;
        const uint32_t sh = (uint32_t)((uintptr_t)src & 15u), head = bytes < ((16u - sh) & 15u) ? bytes : ((16u - sh) & 15u), nvec = (bytes - head) / 16u;
        const uint32_t tail0 = head + nvec * 16u;
        // the stage: exactly the bytes the kernel's holds, poisoned, so that a byte it never wrote shows
        std::vector<uint8_t> stage((16 + kFramesPerGroup * kRsMaxDepth * kRsMaxN + 15) & ~15u, kPoison);
        for (uint32_t t = 0; t < kThreads; ++t) {
            if (t < head) stage[sh + t] = src[t];
            for (uint32_t i = t; i < nvec; i += kThreads) std::memcpy(&stage[sh + head + 16u * i], src + head + 16u * i, 16);
            if (t < bytes - tail0) stage[sh + tail0 + t] = src[tail0 + t];
        }
        for (uint32_t w = 0; w < kWaves; ++w) {
            uint8_t mem[128];
            std::memset(mem, kPoison, sizeof mem);
            uint8_t *S = mem, *lamv = mem + 32, *omv = mem + 80;
            for (uint32_t cw = w; cw < nfr * I; cw += kWaves) {
                const uint32_t fr = cw / I, ci = cw - fr * I;
                uint8_t *word = stage.data() + sh + fr * fbytes;
                uint32_t syn[kWave][kRsMaxRoots / 4], tot[kRsMaxRoots / 4], any = 0;
                for (uint32_t lane = 0; lane < kWave; ++lane) {
                    uint32_t sym = 0;
                    for (uint32_t q = 0; q < 4; ++q) {
                        const uint32_t s = 4 * lane + q;
                        if (s < n) sym |= (uint32_t)word[rs_byte_of(c, ci, s)] << (8 * q);
                    }
                    rs_lane_syndromes(ex, lg, c, sym, lane, syn[lane]);
                }
                for (uint32_t d = 0; d < kRsMaxRoots / 4; ++d) {
                    tot[d] = 0;
                    if (4 * d < nroots)
                        for (uint32_t lane = 0; lane < kWave; ++lane) tot[d] ^= syn[lane][d];
                    any |= tot[d];
                }
                stats[0] += 1;
                uint32_t nerr = 0;
                if (!any) {
                    stats[1] += 1;
                } else {
                    for (uint32_t lane = 0; lane < kRsMaxRoots / 4; ++lane) std::memcpy(S + 4 * lane, &tot[lane], 4);   // (little-endian, as the device)
                    uint32_t lam[kWave] = {1}, bs[kWave] = {1}, b = 1, L = 0;
                    for (uint32_t r = 0; r < nroots; ++r) {
                        for (uint32_t lane = kWave; lane-- > 1;) bs[lane] = bs[lane - 1];
                        bs[0] = 0;
                        uint32_t term[kWave];
                        for (uint32_t lane = 0; lane < kWave; ++lane) term[lane] = rs_bm_term(ex, lg, lam[lane], S, r, lane);
                        const uint32_t d = wave_xor(term), b0 = b, L0 = L;
                        for (uint32_t lane = 0; lane < kWave; ++lane) {
                            uint32_t bl = b0, Ll = L0;
                            rs_bm_update(ex, lg, d, r, bl, Ll, lam[lane], bs[lane]);
                            b = bl;
                            L = Ll;
                        }
                    }
                    nerr = 255;
                    if (2 * L <= nroots) {
                        for (uint32_t lane = 0; lane <= kRsMaxRoots; ++lane) lamv[lane] = (uint8_t)lam[lane];
                        for (uint32_t lane = 0; lane < kRsMaxRoots; ++lane) omv[lane] = lane < L ? (uint8_t)rs_omega(ex, lg, lamv, L, S, lane) : (uint8_t)0;
                        uint32_t roots = 0, found[kWave], zl[kWave][4], val[4];
                        for (uint32_t lane = 0; lane < kWave; ++lane) {
                            found[lane] = 0;
                            for (uint32_t q = 0; q < 4; ++q) zl[lane][q] = 4 * lane + q < n ? rs_zlog(c, 4 * lane + q) : 0u;
                            rs_eval4(ex, lg, lamv, L + 1, zl[lane], 0, 1, val);
                            for (uint32_t q = 0; q < 4; ++q) {
                                const bool root = 4 * lane + q < n && val[q] == 0;
                                found[lane] |= (uint32_t)root << q;
                                roots += root;
                            }
                        }
                        if (roots == L) {
                            nerr = L;
                            for (uint32_t lane = 0; lane < kWave; ++lane)
                                if (found[lane]) {
                                    uint32_t num[4], den[4];
                                    rs_eval4(ex, lg, omv, L, zl[lane], 0, 1, num);
                                    rs_eval4(ex, lg, lamv, L + 1, zl[lane], 1, 2, den);
                                    for (uint32_t q = 0; q < 4; ++q)
                                        if (found[lane] >> q & 1) {
                                            const uint32_t mag = rs_value(ex, lg, c, num[q], den[q], zl[lane][q]);
                                            word[rs_byte_of(c, ci, 4 * lane + q)] ^= (uint8_t)mag;
                                            stats[4] += (uint64_t)__builtin_popcount(mag);
                                        }
                                }
                            stats[3] += L;
                        }
                    }
                    if (nerr == 255) stats[2] += 1;
                }
                nerr_out[(f0 + fr) * I + ci] = (uint8_t)nerr;
            }
        }
        uint8_t *dst = out + f0 * dbytes;
        const uint32_t obytes = nfr * dbytes, al = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u, ohead = obytes < al ? obytes : al, nw = (obytes - ohead) / 4u;
        const uint32_t otail0 = ohead + nw * 4u;
        auto data_byte = [&](uint32_t q) -> uint32_t {
            const uint32_t fr = (uint32_t)(q >= dbytes) + (uint32_t)(q >= 2 * dbytes) + (uint32_t)(q >= 3 * dbytes);
            return stage[sh + fr * fbytes + (q - fr * dbytes)];
        };
        for (uint32_t t = 0; t < kThreads; ++t) {
            if (t < ohead) dst[t] = (uint8_t)data_byte(t);
            for (uint32_t i = t; i < nw; i += kThreads) {
                const uint32_t q = ohead + 4u * i, v = data_byte(q) | data_byte(q + 1) << 8 | data_byte(q + 2) << 16 | data_byte(q + 3) << 24;
                std::memcpy(dst + q, &v, 4);
            }
            if (t < obytes - otail0) dst[otail0 + t] = (uint8_t)data_byte(otail0 + t);
        }
    }
}

void encode(const RsField &F, const RsCode &c, const uint8_t *in, uint64_t nframes, uint8_t *out) {
    const uint32_t I = c.depth, n = c.n, k = c.k;
    for (uint64_t cw = 0; cw < nframes * I; ++cw) {                              // one lane each
        const uint64_t f = cw / I;
        const uint32_t ci = (uint32_t)(cw - f * I);
        const uint8_t *src = in + f * I * k;
        uint8_t *dst = out + f * I * n;
        uint8_t par[kRsMaxRoots] = {0};
        for (uint32_t s = 0; s < k; ++s) {
            const uint32_t d = src[rs_byte_of(c, ci, s)];
            dst[rs_byte_of(c, ci, s)] = (uint8_t)d;
            rs_lfsr_step(F.ex, F.lg, c.gq, par, d);
        }
        for (uint32_t j = 0; j < c.nroots; ++j) dst[rs_byte_of(c, ci, k + j)] = par[j];
    }
}

void hex(FILE *f, const uint8_t *p, size_t nbytes) {
    for (size_t i = 0; i < nbytes; ++i) std::fprintf(f, "%02x", p[i]);
    std::fprintf(f, "\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "w");
    if (!fi || !fo) return 2;
    Case c;
    int ncases = 0;
    while (std::fread(&c, sizeof c, 1, fi) == 1) {
        RsField F;
        RsCode code;
        if (!rs_field((uint32_t)c.prim_poly, F)) std::abort();
        rs_code(F, (uint32_t)c.fcr, (uint32_t)c.prim, (uint32_t)c.nroots, (uint32_t)c.n, (uint32_t)c.depth, code);
        const size_t cb = (size_t)c.nframes * code.depth * code.n, db = (size_t)c.nframes * code.depth * code.k;
        const size_t ib = c.mode ? db : cb, ob = c.mode ? cb : db;
        std::vector<uint8_t> raw((ib + 7) / 8 * 8);
        if (std::fread(raw.data(), 1, raw.size(), fi) != raw.size()) return 3;
        // the buffers as the caller lays them out: exactly the bytes that exist, so that an access outside them is caught
        std::vector<uint8_t> in((size_t)c.in_off + ib, kPoison), out((size_t)c.out_off + ob, kPoison), nerr((size_t)c.nframes * code.depth);
        std::memcpy(in.data() + c.in_off, raw.data(), ib);
        uint64_t stats[5] = {0, 0, 0, 0, 0};
        if (c.mode) encode(F, code, in.data() + c.in_off, (uint64_t)c.nframes, out.data() + c.out_off);
        else decode(F, code, in.data() + c.in_off, (uint64_t)c.nframes, out.data() + c.out_off, nerr.data(), stats);
        for (int64_t i = 0; i < c.out_off; ++i)
            if (out[(size_t)i] != kPoison) return 4;
        std::fprintf(fo, "%llu %llu %llu %llu %llu\n", (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2],
                     (unsigned long long)stats[3], (unsigned long long)stats[4]);
        hex(fo, nerr.data(), c.mode ? 0 : nerr.size());
        hex(fo, out.data() + c.out_off, ob);
        ++ncases;
    }
    std::fclose(fi);
    std::fclose(fo);
    std::printf("cases %d\n", ncases);
    return 0;
}
