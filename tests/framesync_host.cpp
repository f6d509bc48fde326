// framesync_host.cpp -- the kernels' walks of bbb_framesync_run, bbb_frame_extract and bbb_frame_attach restated on the CPU around
// the SAME per-lane core (basebandboard_amd/csrc/framesync_common.hpp): the search pass with a word of 64 positions a lane, the
// next word taken from the lane above (the wave's last lane loads it), one candidate word stored a lane and a flag bit a tile;
// the chain pass as one workgroup of 256 lanes, phase by phase between its barriers -- the flag scan, the flagged tile's candidate
// words, the confirmations in the lanes that hold candidates, the minimum over the lanes, the rejected candidates below it; in
// LOCK four frames a lane, the wave ballots as mask words, the run of misses looked up per lane, the first loss by a minimum,
// the records before it; extract with one aligned output word a lane (whole words inside one payload through the funnel, the
// others byte by byte) and attach with one packed word a lane.  Every buffer is an allocation of exactly its size (the input
// `off` bytes into one), so an access a kernel would make outside its buffers is one AddressSanitizer reports.  Built with
// -fsanitize=address,undefined by tests/test_framesync_host.py, which compares the output with tests/framesync_model.py.
//
//   framesync_host cases.bin out.txt
// cases.bin: per case 15 uint64 (marker, M, F, tol_search, tol_lock, v, w, both, rand_poly, rand_seed, nbits, first_bit, off,
// max_frames, nwords) and nwords words of packed bits.  One final call from a zero state at first_bit.  out.txt gets five lines:
// the eight state words, the positions, the meta words, the extracted payloads in hex and the frames attached again in hex (the
// last two empty where F - M is no multiple of 8).
#include "../basebandboard_amd/csrc/framesync_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bbb;

namespace {

constexpr uint32_t kWave = 64, kWaves = kFsThreads / kWave;
constexpr uint64_t kNone = ~0ull;

uint64_t words_of(uint64_t nbits) { return (nbits + 63) / 64; }
uint64_t tiles_of(uint64_t nbits) { return (words_of(nbits) + kFsTileWords - 1) / kFsTileWords; }
uint64_t flag_words_of(uint64_t nbits) { return (tiles_of(nbits) + 63) / 64; }

// an allocation of exactly n elements (at least one byte, so that the pointer is one)
template <class T> T *exact(uint64_t n, int fill) {
    T *p = (T *)std::malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    std::memset(p, fill, n * sizeof(T));
    return p;
}

void search_pass(const FsCfg &c, const uint64_t *in, uint64_t nbits, uint64_t *flags, uint64_t *plane) {
    const uint64_t nwords = words_of(nbits), ntiles = tiles_of(nbits);
    for (uint64_t i = 0; i < flag_words_of(nbits); ++i) flags[i] = 0;              // the memset in front of the kernel
    for (uint64_t tile = 0; tile < ntiles; ++tile) {
        uint64_t w0[kFsThreads], w1[kFsThreads];
        bool any = false;
        for (uint32_t t = 0; t < kFsThreads; ++t) {
            const uint64_t j = tile * kFsTileWords + t;
            w0[t] = j < nwords ? in[j] : 0;
        }
        for (uint32_t t = 0; t < kFsThreads; ++t) {
            const uint64_t j = tile * kFsTileWords + t;
            const uint32_t lane = t & (kWave - 1);
            w1[t] = lane == kWave - 1 ? (j + 1 < nwords ? in[j + 1] : 0) : w0[t + 1];
            if (j < nwords) {
                const uint64_t valid = fs_valid_mask(j, nbits, c.M);
                const uint64_t cand = valid ? fs_candidate_word(w0[t], w1[t], c) & valid : 0;
                plane[j] = cand;
                any = any || cand;
            }
        }
        if (any) flags[tile >> 6] |= 1ull << (tile & 63);
    }
}

void chain_pass(const FsCfg &c, const uint64_t *in, uint64_t n, uint64_t first_bit, bool final, uint64_t *state, uint64_t *pos, uint16_t *meta,
                uint64_t max_frames, const uint64_t *flags, const uint64_t *plane) {
    const uint64_t nwords = words_of(n), ntiles = tiles_of(n), nfw = flag_words_of(n);
    FsWord0 s = fs_unpack(state[0]);
    if (state[1] < first_bit) {
        state[0] |= 1ull << 25;
        return;
    }
    uint64_t r = state[1] - first_bit, emitted = 0, fly = 0, acq = 0, losses = 0, rej = 0, mbe = 0;
    for (;;) {
        if (s.mode == kFsModeLock) {
            const uint64_t K = fs_lock_steps(r, n, c);
            if (!K) break;
            const uint32_t B = (uint32_t)(K < kFsBatch ? K : kFsBatch);
            static uint32_t d[4][kFsThreads];
            uint64_t mm[kFsMaskWords];
            for (uint32_t q = 0; q < 4; ++q)
                for (uint32_t wv = 0; wv < kWaves; ++wv) {
                    uint64_t bm = 0;
                    for (uint32_t lane = 0; lane < kWave; ++lane) {
                        const uint32_t t = wv * kWave + lane, j = t + kFsThreads * q;
                        d[q][t] = j < B ? fs_dist(in, r + (uint64_t)j * c.F, s.pol, c) : 0u;
                        bm |= (uint64_t)(d[q][t] > c.tol_lock) << lane;
                    }
                    mm[4 * q + wv] = bm;
                }
            uint64_t first_loss = kNone;
            for (uint32_t t = 0; t < kFsThreads; ++t)
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t j = t + kFsThreads * q;
                    if (d[q][t] > c.tol_lock && fs_miss_run(mm, (int32_t)j, s.misses, c.w) > c.w && j < first_loss) first_loss = j;
                }
            const uint32_t carried = fs_miss_run(mm, (int32_t)B - 1, s.misses, c.w);
            const uint32_t L = first_loss == kNone ? B : (uint32_t)first_loss;
            for (uint32_t t = 0; t < kFsThreads; ++t)
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t j = t + kFsThreads * q;
                    if (j >= L) continue;
                    const bool miss = d[q][t] > c.tol_lock;
                    if (emitted + j < max_frames) {
                        pos[emitted + j] = first_bit + r + (uint64_t)j * c.F;
                        meta[emitted + j] = fs_meta(d[q][t], s.pol, miss, s.fresh && j == 0);
                    }
                    fly += miss;
                    if (!miss) mbe += d[q][t];
                }
            emitted += L;
            if (L) s.fresh = 0;
            r += (uint64_t)L * c.F;
            if (L < B) {
                s.mode = kFsModeSearch;
                s.misses = 0;
                ++losses;
            } else {
                s.misses = carried;
            }
        } else {
            if (!fs_search_open(r, n, c)) break;
            const uint64_t tile0 = (r >> 6) / kFsTileWords;
            uint64_t tile = kNone;
            for (uint64_t base = tile0 >> 6; base < nfw && tile == kNone; base += kFsThreads)
                for (uint32_t t = 0; t < kFsThreads; ++t) {
                    const uint64_t i = base + t;
                    uint64_t f = i < nfw ? flags[i] : 0;
                    if (i == tile0 >> 6) f &= ~0ull << (tile0 & 63);
                    if (f && i * 64 + (uint64_t)__builtin_ctzll(f) < tile) tile = i * 64 + (uint64_t)__builtin_ctzll(f);
                }
            if (tile == kNone || tile >= ntiles) {
                r = n - c.M + 1;
                break;
            }
            uint64_t win = kNone, myrej[kFsThreads];
            for (uint32_t t = 0; t < kFsThreads; ++t) {
                const uint64_t j = tile * kFsTileWords + t;
                uint64_t cw = j < nwords ? plane[j] & fs_from_mask(j, r) : 0, res = kNone;
                myrej[t] = 0;
                while (cw) {
                    const uint64_t p = 64 * j + (uint64_t)__builtin_ctzll(cw);
                    cw &= cw - 1;
                    if (!final && !fs_candidate_open(p, n, c)) {
                        res = p << 2 | 3;
                        break;
                    }
                    const uint32_t pol = fs_candidate(fs_dist0(in, p, c), c) - 1;
                    if (fs_confirm(in, p, pol, n, c)) {
                        res = p << 2 | (1 + pol);
                        break;
                    }
                    ++myrej[t];
                }
                if (res < win) win = res;
            }
            for (uint32_t t = 0; t < kFsThreads; ++t) {
                const uint64_t j = tile * kFsTileWords + t;
                if (win == kNone || j <= (win >> 2) >> 6) rej += myrej[t];
            }
            if (win == kNone) {
                r = (tile + 1) * kFsTileBits;
                if (!fs_search_open(r, n, c)) {
                    r = n - c.M + 1;
                    break;
                }
                continue;
            }
            r = win >> 2;
            if ((win & 3) == 3) break;
            s.mode = kFsModeLock;
            s.pol = (uint32_t)(win & 3) - 1;
            s.misses = 0;
            s.fresh = 1;
            ++acq;
        }
    }
    if (emitted > max_frames) s.overflow = 1;
    state[0] = fs_pack(s, emitted);
    state[1] = first_bit + r;
    state[2] += emitted;
    state[3] += fly;
    state[4] += acq;
    state[5] += losses;
    state[6] += rej;
    state[7] += mbe;
}

void table2(const FsRand &R, uint8_t *tab2) {
    for (uint32_t i = 0; i < R.period; ++i) tab2[i] = R.tab[i];
}

void extract(const FsCfg &c, const FsRand &R, const uint64_t *in, uint64_t nbits, uint64_t first_bit, const uint64_t *pos, const uint16_t *meta,
             const uint64_t *state, uint64_t max_frames, uint8_t *out) {
    uint8_t *tab2 = exact<uint8_t>(R.period, 0xA5);
    table2(R, tab2);
    const uint32_t PB = c.payload_bytes;
    const uint64_t count = state[0] >> 32 < max_frames ? state[0] >> 32 : max_frames, total = count * PB;
    auto frame_at = [&](uint64_t fi) -> uint64_t {
        const uint64_t p = pos[fi];
        return p >= first_bit && p - first_bit + c.F <= nbits ? p - first_bit : kNone;
    };
    for (uint64_t q = 0; 8 * q < total; ++q) {
        const uint64_t b = 8 * q, fi = b / PB;
        const uint32_t nb = (uint32_t)(total - b < 8 ? total - b : 8), off = (uint32_t)(b - fi * PB);
        uint64_t x = 0;
        if (off + nb <= PB) {
            const uint64_t p = frame_at(fi);
            if (p != kNone) x = fs_payload_word(in, p, off, nb, meta[fi] >> 8 & 1, c, tab2, R.period);
        } else {
            uint64_t f = fi;
            uint32_t o = off;
            for (uint32_t k = 0; k < nb; ++k) {
                const uint64_t p = frame_at(f);
                if (p != kNone) x |= fs_payload_word(in, p, o, 1, meta[f] >> 8 & 1, c, tab2, R.period) << (8 * k);
                if (++o == PB) {
                    o = 0;
                    ++f;
                }
            }
        }
        if (nb == 8) std::memcpy(out + b, &x, 8);
        else
            for (uint32_t k = 0; k < nb; ++k) out[b + k] = (uint8_t)(x >> (8 * k));
    }
    std::free(tab2);
}

void attach(const FsCfg &c, const FsRand &R, const uint8_t *payload, uint64_t nframes, uint64_t *out) {
    uint8_t *tab2 = exact<uint8_t>(R.period, 0xA5);
    table2(R, tab2);
    const uint64_t nwords = words_of(nframes * c.F);
    for (uint64_t g = 0; g < nwords; ++g) {
        uint64_t fi = 64 * g / c.F, x = 0;
        uint32_t o = (uint32_t)(64 * g - fi * c.F), filled = 0;
        while (filled < 64 && fi < nframes) {
            const uint32_t take = 64u - filled < c.F - o ? 64u - filled : c.F - o;
            x |= fs_frame_bits(payload, fi, o, take, c, tab2, R.period) << filled;
            filled += take;
            o += take;
            if (o == c.F) {
                o = 0;
                ++fi;
            }
        }
        out[g] = x;
    }
    std::free(tab2);
}

void hex(FILE *f, const uint8_t *p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) std::fprintf(f, "%02x", p[i]);
    std::fprintf(f, "\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "w");
    if (!fi || !fo) return 2;
    uint64_t h[15];
    int ncases = 0;
    while (std::fread(h, 8, 15, fi) == 15) {
        FsCfg c{};
        FsRand R;
        c.marker = h[0];
        c.M = (uint32_t)h[1];
        c.mask = c.M == 64 ? ~0ull : (1ull << c.M) - 1;
        c.F = (uint32_t)h[2];
        c.tol_search = (uint32_t)h[3];
        c.tol_lock = (uint32_t)h[4];
        c.v = (uint32_t)h[5];
        c.w = (uint32_t)h[6];
        c.both = (uint32_t)h[7];
        c.payload_bytes = (c.F - c.M) % 8 ? 0 : (c.F - c.M) / 8;
        if (!fs_rand_table((uint32_t)h[8], (uint32_t)h[9], R)) return 3;
        const uint64_t nbits = h[10], first_bit = h[11], off = h[12], max_frames = h[13], nwords = h[14];
        if (nwords != words_of(nbits)) return 3;
        uint8_t *raw = exact<uint8_t>(off + 8 * nwords, 0xA5);
        if (nwords && std::fread(raw + off, 8, nwords, fi) != nwords) return 3;
        const uint64_t *in = (const uint64_t *)(raw + off);
        uint64_t *flags = exact<uint64_t>(flag_words_of(nbits) + nwords, 0xA5), *plane = flags + flag_words_of(nbits);
        uint64_t *pos = exact<uint64_t>(max_frames, 0xA5);
        uint16_t *meta = exact<uint16_t>(max_frames, 0xA5);
        uint64_t state[8] = {0, first_bit, 0, 0, 0, 0, 0, 0};
        search_pass(c, in, nbits, flags, plane);
        chain_pass(c, in, nbits, first_bit, true, state, pos, meta, max_frames, flags, plane);
        const uint64_t count = state[0] >> 32 < max_frames ? state[0] >> 32 : max_frames;
        for (int i = 0; i < 8; ++i) std::fprintf(fo, "%llu ", (unsigned long long)state[i]);
        std::fprintf(fo, "\n");
        for (uint64_t i = 0; i < count; ++i) std::fprintf(fo, "%llu ", (unsigned long long)pos[i]);
        std::fprintf(fo, "\n");
        for (uint64_t i = 0; i < count; ++i) std::fprintf(fo, "%u ", (unsigned)meta[i]);
        std::fprintf(fo, "\n");
        if (c.payload_bytes) {
            uint8_t *pay = exact<uint8_t>(max_frames * c.payload_bytes, 0xA5);
            extract(c, R, in, nbits, first_bit, pos, meta, state, max_frames, pay);
            hex(fo, pay, count * c.payload_bytes);
            uint64_t *back = exact<uint64_t>(words_of(count * c.F), 0xA5);
            attach(c, R, pay, count, back);
            hex(fo, (const uint8_t *)back, 8 * words_of(count * c.F));
            std::free(pay);
            std::free(back);
        } else {
            std::fprintf(fo, "\n\n");
        }
        std::free(raw);
        std::free(flags);
        std::free(pos);
        std::free(meta);
        ++ncases;
    }
    std::fclose(fi);
    std::fclose(fo);
    std::printf("cases %d\n", ncases);
    return 0;
}
