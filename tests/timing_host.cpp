// timing_host.cpp -- the three passes of bbb_timing_run restated on the CPU, thread by thread, over the shared core of
// basebandboard_amd/csrc/timing_common.hpp, and compared with the definition written as a plain serial loop.  Built with
// -fsanitize=address,undefined and run as a program by tests/test_timing_host.py, which compares what it prints with
// tests/timing_model.py.
//
//   timing_host cases.bin out.txt
// A case: int64 head[12] = {n, P, L, h, threshold, strict, init_phase, chunk, state0, state1, final, 0}, then int32 a[n + 1]
// (a(-1) first) padded to a multiple of 8 bytes.  The filter is not restated here: the passes take a(n) as given.
#include "../basebandboard_amd/csrc/timing_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bbb;

namespace {

struct Case {
    TimingGeom g;
    int32_t threshold;
    bool strict;
    uint32_t init;
    uint64_t state[2];
    std::vector<int32_t> a;                        // a[t + 1] = a(t)
    int32_t at(int64_t t) const { return a[(size_t)(t + 1)]; }
};

struct Result {
    uint64_t state[2], nbits = 0, stats[4] = {0, 0, 0, 0};
    std::vector<uint64_t> bits;
    std::vector<int32_t> soft;
    std::vector<uint8_t> phase;
    bool operator==(const Result &o) const {
        return state[0] == o.state[0] && state[1] == o.state[1] && nbits == o.nbits && !memcmp(stats, o.stats, sizeof stats) && bits == o.bits &&
               soft == o.soft && phase == o.phase;
    }
};

uint64_t max_bits(const TimingGeom &g) { return g.nblocks * (g.L + 1); }

// ---- the definition ---------------------------------------------------------------------------------------------------------
Result plain(const Case &c) {
    const TimingGeom &g = c.g;
    Result r;
    r.bits.assign((max_bits(g) + 63) / 64, 0);
    r.soft.assign(max_bits(g), 0);
    r.phase.assign(g.nblocks, 0);
    bool locked = c.state[0] >> 63;
    uint64_t phi = (c.state[0] & 0xFFFFFFFFull) % g.P;
    std::vector<int64_t> E(g.P);
    for (uint64_t j = 0; j < g.nblocks; ++j) {
        for (uint32_t p = 0; p < g.P; ++p) {
            E[p] = 0;
            for (uint32_t i = 0; i < g.L; ++i) {
                const uint64_t t = j * g.LP + (uint64_t)i * g.P + p;
                if (t < g.nin) E[p] += std::llabs((long long)c.at((int64_t)t) - c.threshold);
            }
        }
        int m = 0, w = 0;
        if (!locked) {
            phi = 0;
            if (c.init < g.P) phi = c.init;
            else
                for (uint32_t p = 1; p < g.P; ++p)
                    if (E[p] > E[phi]) phi = p;
            locked = true;
        } else {
            const int64_t cur = E[phi], up = E[(phi + 1) % g.P], dn = E[(phi + g.P - 1) % g.P], margin = cur >> g.h;
            if (up > cur + margin && up >= dn) m = 1;
            else if (dn > cur + margin) m = -1;
            phi = (phi + g.P + m) % g.P;
            if (m == 1 && phi == 0) w = 1;
            if (m == -1 && phi == g.P - 1) w = -1;
        }
        r.phase[j] = (uint8_t)phi;
        r.stats[0]++;
        r.stats[1] += m != 0;
        r.stats[2] += w > 0;
        r.stats[3] += w < 0;
        for (int64_t i = w; i < (int64_t)g.L; ++i) {
            const int64_t t = (int64_t)(j * g.LP + phi) + i * (int64_t)g.P;
            if (t >= (int64_t)g.nin) break;
            const int32_t v = c.at(t);
            r.bits[r.nbits >> 6] |= (uint64_t)(c.strict ? v > c.threshold : v >= c.threshold) << (r.nbits & 63);
            r.soft[r.nbits++] = v;
        }
    }
    r.state[0] = g.nblocks ? kTimingLocked | phi : c.state[0];
    r.state[1] = c.state[1] + r.nbits;
    return r;
}

// ---- the passes, as the kernels walk them -------------------------------------------------------------------------------------
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(2);                                                      \
        }                                                                 \
    } while (0)

Result passes(const Case &c) {
    const TimingGeom &g = c.g;
    const uint32_t P = g.P, T = timing_tiles_per_block(g.LP), split = timing_split(P, g.LP);
    Result r;
    r.bits.assign((max_bits(g) + 63) / 64, 0);
    r.soft.assign(max_bits(g), 0);
    r.phase.assign(g.nblocks, 0);
    std::vector<uint8_t> mv(g.nblocks * P), cmap(g.nchunks * P), cstart(g.nchunks);
    std::vector<uint32_t> cbits(g.nchunks * P);
    std::vector<uint64_t> boff(g.nblocks), coff(g.nchunks);
    std::vector<uint16_t> binfo(g.nblocks);
    uint64_t argmax0 = 0;
    CHECK(split >= 1 && (split & (split - 1)) == 0 && split * timing_blocks_per_tile(g.LP) * P <= (uint32_t)kTimingThreads);

    // the metric pass: a group of tiles per workgroup step, `split` threads per (block, phase) pair
    for (uint64_t grp = 0; grp < timing_ngroups(g); ++grp) {
        std::vector<uint64_t> sum(kTimingThreads, 0), E(kTimingThreads, 0);
        TimingTile tl{};
        for (uint32_t o = 0; o < T; ++o) {
            tl = timing_tile(g, grp * T + o);
            CHECK(tl.len <= kTimingTile && tl.nblk * P <= (uint32_t)kTimingThreads);
            uint32_t vals[kTimingTile];
            for (uint32_t k = 0; k < kTimingTile; ++k) vals[k] = tl.base + k < g.nin ? timing_term(c.at((int64_t)(tl.base + k)), c.threshold) : 0u;
            for (uint32_t t = 0; t < (uint32_t)kTimingThreads; ++t) {
                const uint32_t pair = t / split, s = t % split, jb = pair / P, p = pair % P;
                if (jb >= tl.nblk) continue;
                uint32_t k0, kend;
                timing_pair_span(g, tl, jb, p, k0, kend);
                CHECK(kend <= kTimingTile);
                for (uint32_t k = k0 + s * P; k < kend; k += split * P) sum[t] += vals[k];
            }
        }
        for (uint32_t d = split >> 1; d; d >>= 1) {                       // the lanes' butterfly
            std::vector<uint64_t> nxt(sum);
            for (uint32_t t = 0; t < (uint32_t)kTimingThreads; ++t) nxt[t] = sum[t] + sum[t ^ d];
            sum = nxt;
        }
        for (uint32_t t = 0; t < (uint32_t)kTimingThreads; t += split)
            if (t / split / P < tl.nblk) E[t / split] = sum[t];
        for (uint32_t t = 0; t < tl.nblk * P; ++t) mv[(tl.j0 + t / P) * P + t % P] = (uint8_t)(timing_move_at(E.data() + t / P * P, P, t % P, g.h) + 1);
        if (tl.j0 == 0) argmax0 = timing_argmax(E.data(), P);
    }

    // the chunk walk: one lane per start phase
    const bool unlocked = !(c.state[0] & kTimingLocked);
    const uint32_t first_phi = c.init < P ? c.init : (uint32_t)argmax0;
    for (uint64_t ch = 0; ch < g.nchunks; ++ch) {
        const uint64_t j_lo = ch * g.chunk, j_hi = j_lo + g.chunk < g.nblocks ? j_lo + g.chunk : g.nblocks;
        for (uint32_t t = 0; t < P; ++t) {
            uint32_t phi = t, nb = 0;
            for (uint64_t j = j_lo; j < j_hi; ++j) {
                int m, w;
                nb += timing_walk_block(g, j, unlocked && j == 0, first_phi, mv[j * P + phi], phi, m, w);
            }
            cmap[ch * P + t] = (uint8_t)phi;
            cbits[ch * P + t] = nb;
        }
    }

    // the chain: shares of chunks, one serial walk over the shares' totals, the replay
    const uint32_t CT = timing_chain_threads(P);
    const uint64_t share = timing_chain_share(g.nchunks, P);
    CHECK(CT * P <= kTimingChainSlots && CT >= 1 && share * CT >= g.nchunks);
    std::vector<uint8_t> totmap(CT * P), start(CT);
    std::vector<uint64_t> totbits(CT * P), soff(CT);
    auto lo_of = [&](uint32_t t) { return t * share < g.nchunks ? t * share : g.nchunks; };
    for (uint32_t t = 0; t < CT; ++t)
        for (uint32_t phi0 = 0; phi0 < P; ++phi0) {
            uint32_t phi = phi0;
            uint64_t nb = 0;
            for (uint64_t ch = lo_of(t); ch < lo_of(t + 1); ++ch) timing_compose(cmap.data(), cbits.data(), ch, P, phi, nb);
            totmap[t * P + phi0] = (uint8_t)phi;
            totbits[t * P + phi0] = nb;
        }
    uint32_t phi = timing_state_phi(c.state[0], P);
    uint64_t off = 0;
    for (uint32_t k = 0; k < CT; ++k) {
        start[k] = (uint8_t)phi;
        soff[k] = off;
        off += totbits[k * P + phi];
        phi = totmap[k * P + phi];
    }
    r.state[0] = g.nblocks ? kTimingLocked | phi : c.state[0];
    r.state[1] = c.state[1] + off;
    r.nbits = off;
    r.stats[0] = g.nblocks;
    for (uint32_t t = 0; t < CT; ++t) {
        uint32_t ph = start[t];
        uint64_t o = soff[t];
        for (uint64_t ch = lo_of(t); ch < lo_of(t + 1); ++ch) {
            cstart[ch] = (uint8_t)ph;
            coff[ch] = o;
            timing_compose(cmap.data(), cbits.data(), ch, P, ph, o);
        }
    }

    // every chunk once more from its true start
    for (uint64_t ch = 0; ch < g.nchunks; ++ch) {
        const uint64_t j_lo = ch * g.chunk, j_hi = j_lo + g.chunk < g.nblocks ? j_lo + g.chunk : g.nblocks;
        uint32_t ph = cstart[ch];
        uint64_t o = coff[ch];
        for (uint64_t j = j_lo; j < j_hi; ++j) {
            int m, w;
            const uint32_t cnt = timing_walk_block(g, j, unlocked && j == 0, first_phi, mv[j * P + ph], ph, m, w);
            r.phase[j] = (uint8_t)ph;
            boff[j] = o;
            binfo[j] = timing_info(ph, w);
            o += cnt;
            r.stats[1] += m != 0;
            r.stats[2] += w > 0;
            r.stats[3] += w < 0;
        }
    }

    // the gather pass: a tile's instants are consecutive output bits, a thread takes one, a wave's ballot goes into two words
    for (uint64_t tile = 0; tile < timing_ntiles(g); ++tile) {
        const TimingTile tl = timing_tile(g, tile);
        std::vector<uint64_t> seg_start(tl.nblk + 1);
        std::vector<int> seg_ilo(tl.nblk);
        std::vector<uint32_t> seg_phi(tl.nblk);
        for (uint32_t t = 0; t < tl.nblk; ++t) {
            const uint32_t ph = timing_info_phi(binfo[tl.j0 + t]);
            const int w = timing_info_wrap(binfo[tl.j0 + t]);
            int ilo, ihi;
            timing_tile_instants(g, tl, tl.j0 + t, ph, w, ilo, ihi);
            seg_start[t] = boff[tl.j0 + t] + (uint64_t)(ilo - w);
            seg_ilo[t] = ilo;
            seg_phi[t] = ph;
            if (t) CHECK(seg_start[t] >= seg_start[t - 1]);
            if (t == tl.nblk - 1) seg_start[tl.nblk] = boff[tl.j0 + t] + (uint64_t)(ihi - w);
        }
        const uint64_t lo = seg_start[0];
        const uint32_t n = (uint32_t)(seg_start[tl.nblk] - lo);
        for (uint32_t r0 = 0; r0 < n; r0 += 64) {                          // one wave's round
            uint64_t bal = 0, vmask = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t q = r0 + lane;
                if (q >= n) continue;
                CHECK(lo + q < max_bits(g));
                uint32_t b0 = 0, b1 = tl.nblk;
                while (b1 - b0 > 1) {
                    const uint32_t mid = (b0 + b1) / 2;
                    if ((uint32_t)(seg_start[mid] - lo) <= q) b0 = mid;
                    else b1 = mid;
                }
                const int i = seg_ilo[b0] + (int)(q - (uint32_t)(seg_start[b0] - lo));
                const int k = (int)(b0 * g.LP) - (int)tl.off + (int)seg_phi[b0] + i * (int)P;
                CHECK(k >= -1 && k < (int)kTimingTile && (int64_t)tl.base + k < (int64_t)g.nin);
                const int32_t v = c.at((int64_t)tl.base + k);
                vmask |= 1ull << lane;
                bal |= (uint64_t)(c.strict ? v > c.threshold : v >= c.threshold) << lane;
                r.soft[lo + q] = v;
            }
            const uint64_t pos = lo + r0;
            const unsigned sh = pos & 63;
            CHECK(!(r.bits[pos >> 6] & (vmask << sh)));                    // nobody wrote these bits before
            r.bits[pos >> 6] |= bal << sh;
            if (sh && (bal >> (64 - sh))) r.bits[(pos >> 6) + 1] |= bal >> (64 - sh);
        }
    }
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "w");
    if (!f || !out) return 1;
    int ncases = 0;
    int64_t head[12];
    while (fread(head, sizeof head, 1, f) == 1) {
        Case c;
        const uint64_t n = (uint64_t)head[0];
        c.g.P = (uint32_t)head[1];
        c.g.L = (uint32_t)head[2];
        c.g.h = (uint32_t)head[3];
        c.threshold = (int32_t)head[4];
        c.strict = head[5] != 0;
        c.init = (uint32_t)head[6];
        c.g.chunk = (uint32_t)head[7];
        c.state[0] = (uint64_t)head[8];
        c.state[1] = (uint64_t)head[9];
        c.g.LP = c.g.L * c.g.P;
        uint64_t nconsumed, mb;
        timing_plan(c.g.P, c.g.L, n, head[10] != 0, c.g.nblocks, nconsumed, mb);
        c.g.nin = nconsumed;
        c.g.nchunks = (c.g.nblocks + c.g.chunk - 1) / c.g.chunk;
        c.a.resize((n + 2) / 2 * 2);
        if (fread(c.a.data(), 4, c.a.size(), f) != c.a.size()) return 1;
        c.a.resize(n + 1);
        if (mb != c.g.nblocks * (c.g.L + 1)) return 3;
        const Result want = plain(c), got = passes(c);
        if (!(want == got)) {
            fprintf(stderr, "case %d: the passes differ from the plain loop (nbits %llu / %llu)\n", ncases, (unsigned long long)got.nbits,
                    (unsigned long long)want.nbits);
            return 4;
        }
        fprintf(out, "%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)got.state[0], (unsigned long long)got.state[1],
                (unsigned long long)got.nbits, (unsigned long long)got.stats[0], (unsigned long long)got.stats[1], (unsigned long long)got.stats[2],
                (unsigned long long)got.stats[3]);
        for (uint64_t w : got.bits) fprintf(out, "%llx ", (unsigned long long)w);
        fprintf(out, "\n");
        for (uint8_t p : got.phase) fprintf(out, "%u ", p);
        fprintf(out, "\n");
        for (uint64_t i = 0; i < got.nbits; ++i) fprintf(out, "%d ", got.soft[i]);
        fprintf(out, "\n");
        ++ncases;
    }
    fclose(out);
    printf("cases %d\n", ncases);
    return 0;
}
