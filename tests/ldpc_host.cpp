// ldpc_host.cpp -- the kernels' walk of bbb_ldpc_decode and bbb_ldpc_encode restated on the CPU around the SAME per-check core
// (basebandboard_amd/csrc/ldpc_common.hpp): workgroups of 256 lanes that take a group of G codewords, stage their values from
// their unaligned start (single halfwords up to the first and behind the last 16-byte boundary, 16-byte pieces between) into an
// "LDS" of exactly ldpc_lds() bytes, pack the hard decisions 64 at a time, raise the syndrome flags, walk the layers lane by lane
// and round by round with the compressed records in that LDS, and gather every output word from the flat bit array, storing
// the words inside the group's bits and OR-ing the shared ones into zeroed memory; and the encoder's walk, one codeword per
// workgroup.  Built with -fsanitize=address,undefined by tests/test_ldpc_host.py, which compares the output with
// tests/ldpc_model.py.
//
//   ldpc_host cases.bin out.txt
// cases.bin: per case 12 int64 (mode, Z, J, K, max_iter, norm, hard_mag, ncodewords, in_first, format, in_off, out_off), the base
// matrix as J K int16 (padded to a multiple of 8 bytes) and the input (padded likewise).  mode 0, decode: the input is the
// buffer of in_first + ncodewords n int16 values (format 0) or that many packed bits (format 1), placed in_off halfwords (or
// words) behind an allocation's start, the output out_off words behind another's; out.txt gets a line with the five statistics,
// a line with iters in hex and a line with the packed data in hex.  mode 1, encode: the input is the packed data bits; out.txt
// gets "0 0 0 0 0", an empty line and the packed coded bits in hex.
#include "../basebandboard_amd/csrc/ldpc_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bbb;

namespace {

constexpr uint32_t kWave = 64, kThreads = kLdpcThreads;
constexpr uint8_t kPoison = 0xA5;

struct Case {
    int64_t mode, Z, J, K, max_iter, norm, hard_mag, ncw, in_first, format, in_off, out_off;
};

// ballot by ballot: the hard decisions of P[0 .. vals)
void pack_hard(const int16_t *P, uint32_t vals, uint64_t *dst) {
    for (uint32_t wave = 0; wave < kThreads / kWave; ++wave)
        for (uint32_t base = wave * kWave; base < vals; base += kThreads) {
            uint64_t mask = 0;
            for (uint32_t lane = 0; lane < kWave; ++lane)
                if (base + lane < vals && P[base + lane] > 0) mask |= 1ull << lane;
            dst[base >> 6] = mask;
        }
}

void store_words(const uint64_t *flat, uint64_t *out, uint64_t b0, uint64_t b1, uint64_t item0, uint32_t per, uint32_t stride) {
    for (uint32_t t = 0; t < kThreads; ++t)
        for (uint64_t W = (b0 >> 6) + t; 64 * W < b1; W += kThreads) {
            const uint64_t v = ldpc_out_word(flat, W, b0, b1, item0, per, stride);
            if (ldpc_word_inside(W, b0, b1)) out[W] = v;
            else if (v) out[W] |= v;
        }
}

void decode(const LdpcCode &c, const void *in, uint64_t in_first, int format, uint64_t ncw, uint64_t *out, uint8_t *iters_out, uint64_t stats[5]) {
    const LdpcLds L = ldpc_lds(c);
    const uint32_t Z = c.Z, J = c.J, n = c.n, m = c.m, k = c.k, G = c.group;
    std::memset(out, 0, 8 * ((ncw * k + 63) / 64));
    const uint64_t ngrp = (ncw + G - 1) / G;
    for (uint64_t grp = 0; grp < ngrp; ++grp) {
        // the LDS: exactly the bytes the kernel's holds, poisoned, so that a byte it never wrote shows
        std::vector<uint64_t> mem((L.bytes + 7) / 8);
        unsigned char *lds = reinterpret_cast<unsigned char *>(mem.data());
        std::memset(lds, kPoison, L.bytes);
        int16_t *Pb = reinterpret_cast<int16_t *>(lds + L.P);
        uint32_t *rec = reinterpret_cast<uint32_t *>(lds + L.rec);
        uint8_t *i1v = lds + L.i1;
        uint64_t *orig = reinterpret_cast<uint64_t *>(lds + L.orig), *fin = reinterpret_cast<uint64_t *>(lds + L.fin);
        int32_t *iters = reinterpret_cast<int32_t *>(lds + L.tab), *bad = iters + kLdpcMaxGroup;
        const uint64_t cw0 = grp * G;
        const uint32_t ng = (uint32_t)(ncw - cw0 < G ? ncw - cw0 : G), vals = ng * n, nchk = ng * Z;
        uint32_t sh = 0;
        if (format == 0) {
            const int16_t *src = reinterpret_cast<const int16_t *>(in) + in_first + cw0 * n;
            sh = (uint32_t)((uintptr_t)src & 15u) / 2u;
            const uint32_t al = (8u - sh) & 7u, head = vals < al ? vals : al, nvec = (vals - head) / 8u, tail0 = head + nvec * 8u;
            int16_t *P = Pb + sh;
            for (uint32_t t = 0; t < kThreads; ++t) {
                if (t < head) P[t] = (int16_t)ldpc_clamp(src[t]);
                for (uint32_t i = t; i < nvec; i += kThreads) {
                    if (((uintptr_t)(src + head + 8u * i) & 15u) || ((uintptr_t)((P + head + 8u * i) - Pb) * 2u & 15u)) std::abort();
                    for (uint32_t h = 0; h < 8; ++h) P[head + 8u * i + h] = (int16_t)ldpc_clamp(src[head + 8u * i + h]);
                }
                if (t < vals - tail0) P[tail0 + t] = (int16_t)ldpc_clamp(src[tail0 + t]);
            }
        } else {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(in);
            const uint64_t bit0 = in_first + cw0 * n;
            for (uint32_t q = 0; q < vals; ++q) {
                const uint64_t b = bit0 + q;
                Pb[q] = (int16_t)((src[b >> 6] >> (b & 63u) & 1u) ? (int32_t)c.hard_mag : -(int32_t)c.hard_mag);
            }
        }
        int16_t *P = Pb + sh;
        for (uint32_t t = 0; t < ng; ++t) {
            iters[t] = kLdpcRunning;
            bad[t] = 0;
        }
        auto syndrome = [&]() {
            for (uint32_t q = 0; q < nchk; ++q) {                               // lane q % 256, round q / 256
                const uint32_t g = q / Z, r = q - g * Z;
                if (iters[g] != kLdpcRunning) continue;
                uint32_t fail = 0;
                for (uint32_t j = 0; j < J; ++j) fail |= ldpc_parity(c, j, r, P + g * n);
                if (fail) bad[g] = 1;
            }
        };
        pack_hard(P, vals, orig);
        syndrome();
        for (uint32_t t = 0; t < ng; ++t)
            if (!bad[t]) iters[t] = 0;
        for (uint32_t it = 0; it < c.max_iter; ++it) {
            uint32_t any = 0;
            for (uint32_t g = 0; g < ng; ++g) any |= (uint32_t)(iters[g] == kLdpcRunning);
            if (!any) break;
            for (uint32_t t = 0; t < ng; ++t) bad[t] = 0;
            for (uint32_t j = 0; j < J; ++j)
                for (uint32_t t = 0; t < kThreads; ++t)
                    for (uint32_t rd = 0; rd < kLdpcRounds; ++rd) {
                        const uint32_t q = t + kThreads * rd;
                        if (q >= nchk) continue;
                        const uint32_t g = q / Z, r = q - g * Z, at = g * m + j * Z + r;
                        if (iters[g] != kLdpcRunning) continue;
                        uint32_t w0 = 0, mask = 0, i1 = 0;
                        if (it) {
                            w0 = rec[2 * at];
                            mask = rec[2 * at + 1];
                            i1 = i1v[at];
                        }
                        ldpc_check(c, j, r, it == 0, P + g * n, w0, mask, i1);
                        rec[2 * at] = w0;
                        rec[2 * at + 1] = mask;
                        i1v[at] = (uint8_t)i1;
                    }
            syndrome();
            for (uint32_t t = 0; t < ng; ++t)
                if (iters[t] == kLdpcRunning && !bad[t]) iters[t] = (int32_t)(it + 1);
        }
        for (uint32_t t = 0; t < ng; ++t)
            if (iters[t] == kLdpcRunning) iters[t] = (int32_t)kLdpcFailed;
        pack_hard(P, vals, fin);
        for (uint32_t g = 0; g < ng; ++g) {
            const int32_t v = iters[g];
            stats[0] += 1;
            if (v == 0) stats[1] += 1;
            else if (v == (int32_t)kLdpcFailed) stats[2] += 1;
            else stats[3] += (uint64_t)v;
            iters_out[cw0 + g] = (uint8_t)v;
        }
        for (uint32_t w = 0; w < (vals + 63u) / 64u; ++w) stats[4] += ldpc_corrected(orig[w] ^ fin[w], w, n, vals, iters);
        store_words(fin, out, cw0 * k, (cw0 + ng) * k, cw0, k, n);
    }
}

void encode(const LdpcCode &c, const uint64_t *src, uint64_t ncw, uint64_t *out) {
    const uint32_t Z = c.Z, n = c.n, k = c.k;
    std::memset(out, 0, 8 * ((ncw * n + 63) / 64));
    for (uint64_t w = 0; w < ncw; ++w) {
        std::vector<int16_t> x(n, (int16_t)0x5A5A);
        std::vector<uint64_t> flat((n + 63) / 64, 0xA5A5A5A5A5A5A5A5ull);
        for (uint32_t i = 0; i < k; ++i) {
            const uint64_t b = w * k + i;
            x[i] = (int16_t)(src[b >> 6] >> (b & 63u) & 1u);
        }
        for (uint32_t j = c.J; j-- > 0;) {
            const uint32_t d = ldpc_diag(c, j);
            if (d == kLdpcMaxDeg) std::abort();
            for (uint32_t r = 0; r < Z; ++r) {
                uint32_t v = 0;
                for (uint32_t e = 0; e < c.deg[j]; ++e)
                    if (e != d) v ^= (uint32_t)x[ldpc_var(c, j, e, r)];
                x[ldpc_var(c, j, d, r)] = (int16_t)v;
            }
        }
        pack_hard(x.data(), n, flat.data());
        store_words(flat.data(), out, w * n, (w + 1) * n, w, n, n);
    }
}

void hex(FILE *f, const void *p, size_t nbytes) {
    for (size_t i = 0; i < nbytes; ++i) std::fprintf(f, "%02x", ((const uint8_t *)p)[i]);
    std::fprintf(f, "\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "w");
    if (!fi || !fo) return 2;
    Case cs;
    int ncases = 0;
    while (std::fread(&cs, sizeof cs, 1, fi) == 1) {
        std::vector<int16_t> base(((size_t)(cs.J * cs.K) + 3) / 4 * 4);
        if (std::fread(base.data(), 2, base.size(), fi) != base.size()) return 3;
        LdpcCode code;
        if (!ldpc_code((uint32_t)cs.Z, (uint32_t)cs.J, (uint32_t)cs.K, base.data(), code)) std::abort();
        code.max_iter = (uint32_t)cs.max_iter;
        code.norm = (uint32_t)cs.norm;
        code.hard_mag = (uint32_t)cs.hard_mag;
        const uint64_t ncw = (uint64_t)cs.ncw, nvals = (uint64_t)cs.in_first + ncw * code.n;
        const size_t ibytes = cs.mode ? 8 * ((ncw * code.k + 63) / 64) : (cs.format ? 8 * ((nvals + 63) / 64) : (2 * nvals + 7) / 8 * 8);
        const size_t iexact = cs.mode || cs.format ? ibytes : 2 * nvals;        // the bytes that exist for the kernel
        const size_t owords = (ncw * (cs.mode ? code.n : code.k) + 63) / 64;
        std::vector<uint8_t> raw(ibytes);
        if (std::fread(raw.data(), 1, raw.size(), fi) != raw.size()) return 3;
        // the buffers as the caller lays them out: exactly the bytes that exist, so that an access outside them is caught
        const size_t unit = cs.mode || cs.format ? 8 : 2;
        // (malloc is 16-byte aligned: in_off moves the base, and with in_first the first value, across the 16-byte phases;
        // there is no slack behind the last value)
        uint8_t *in_tight = (uint8_t *)std::malloc((size_t)cs.in_off * unit + iexact);
        if (!in_tight) return 5;
        std::memcpy(in_tight + (size_t)cs.in_off * unit, raw.data(), iexact);
        std::vector<uint64_t> out((size_t)cs.out_off + owords, 0xA5A5A5A5A5A5A5A5ull);
        std::vector<uint8_t> iters(ncw);
        uint64_t stats[5] = {0, 0, 0, 0, 0};
        if (cs.mode) encode(code, reinterpret_cast<const uint64_t *>(in_tight + (size_t)cs.in_off * unit), ncw, out.data() + cs.out_off);
        else decode(code, in_tight + (size_t)cs.in_off * unit, (uint64_t)cs.in_first, (int)cs.format, ncw, out.data() + cs.out_off, iters.data(), stats);
        std::free(in_tight);
        for (int64_t i = 0; i < cs.out_off; ++i)
            if (out[(size_t)i] != 0xA5A5A5A5A5A5A5A5ull) return 4;
        std::fprintf(fo, "%llu %llu %llu %llu %llu\n", (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2],
                     (unsigned long long)stats[3], (unsigned long long)stats[4]);
        hex(fo, iters.data(), cs.mode ? 0 : iters.size());
        hex(fo, out.data() + cs.out_off, 8 * owords);
        ++ncases;
    }
    std::fclose(fi);
    std::fclose(fo);
    std::printf("cases %d\n", ncases);
    return 0;
}
