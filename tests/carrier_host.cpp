// carrier_host.cpp -- the five passes of basebandboard_amd/csrc/carrier_kernels.hip restated on the CPU, thread by thread, over
// basebandboard_amd/csrc/carrier_common.hpp (the per-pair square, the normalisation, h, near, the rotate step and the tile and
// block arithmetic).  Built stand-alone with -fsanitize=address,undefined by tests/test_carrier_host.py, which hands it cases
// and compares what it prints with tests/carrier_model.py and bbb_carrier_model_host.  Every case is also held, here, to a
// plain serial loop of the definition.
//
//   carrier_host cases.bin out.txt
// cases.bin: per case nine int64 (npairs, L, init_phase, threshold, strict, chunk, state0, state1, final), then npairs pairs
// of int16 padded to a multiple of 8 bytes.  out.txt, per case: "state0 state1 stats[4]" / the bit words in hex / the phases /
// the pairs turned back / the soft values.
#include "../basebandboard_amd/csrc/carrier_common.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bbb;

namespace {

constexpr int kWave = 64;

struct Case {
    uint32_t L, init, strict, chunk;
    int32_t threshold;
    uint64_t state[2];
    bool final;
    std::vector<int16_t> in;                       // 2 * npairs
};

struct Result {
    uint64_t state[2], stats[4];
    std::vector<uint64_t> words;
    std::vector<uint16_t> phases;
    std::vector<int16_t> iq, soft;
};

int16_t rom[1024];

// the NCO's ROM: round(sin(linspace(0, 2 pi, 1024)) * 32767), read from the file the test writes
void load_rom(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(rom, 2, 1024, f) != 1024) {
        std::fprintf(stderr, "cannot read the ROM\n");
        std::exit(2);
    }
    std::fclose(f);
}

// a thread's 8 pairs with zeros from nin on, as carrier_load gives them
void load8(const Case &c, uint64_t nin, uint64_t p0, bool active, int (&i)[8], int (&q)[8]) {
    for (int k = 0; k < 8; ++k) {
        const bool in = active && p0 + k < nin;
        i[k] = in ? c.in[2 * (p0 + k)] : 0;
        q[k] = in ? c.in[2 * (p0 + k) + 1] : 0;
    }
}

Result passes(const Case &c) {
    Result r{};
    CarrierGeom g{};
    g.L = c.L;
    g.chunk = c.chunk;
    uint64_t nconsumed;
    carrier_plan(c.L, c.in.size() / 2, c.final, g.nblocks, nconsumed);
    g.nin = nconsumed;
    g.nchunks = (g.nblocks + g.chunk - 1) / g.chunk;
    r.words.assign(carrier_bit_words(g.nblocks, g.L), 0xA5A5A5A5A5A5A5A5ull);
    r.phases.assign(g.nblocks, 0xEEEE);
    r.iq.assign(2 * g.nin, 0x5A5A);
    r.soft.assign(g.nin, 0x5A5A);
    std::memset(r.stats, 0, sizeof r.stats);
    std::vector<uint16_t> h(g.nblocks), e(g.nblocks);
    std::vector<uint8_t> cpar(g.nchunks), cstart(g.nchunks);
    const uint32_t L8 = g.L / 8, G = carrier_blocks_per_tile(g.L), fold = carrier_fold(g.L), per = L8 / fold, T = kCarrierThreads;
    const uint64_t ntiles = carrier_ntiles(g);
    if ((L8 % fold) || fold > 64 || (kWave % fold) || G * L8 > T || carrier_tile_pairs(g.L) != G * g.L) std::abort();

    // ---- the sum pass
    for (uint64_t tile = 0; tile < ntiles; ++tile) {
        const uint64_t j0 = tile * G, base = j0 * g.L;
        const uint32_t nblk = (uint32_t)(g.nblocks - j0 < G ? g.nblocks - j0 : G);
        std::vector<int64_t> tr(T), ti(T), pr(T), pi(T);
        for (uint32_t t = 0; t < T; ++t) {
            int i[8], q[8];
            load8(c, g.nin, base + 8 * t, t < G * L8, i, q);
            int64_t sr = 0, siq = 0;
            for (int k = 0; k < 8; ++k) carrier_square(i[k], q[k], sr, siq);
            tr[t] = sr;
            ti[t] = siq;
        }
        for (uint32_t d = fold >> 1; d; d >>= 1) {     // the shuffles: every lane adds its partner's value of the step before
            std::vector<int64_t> nr(T), ni(T);
            for (uint32_t t = 0; t < T; ++t) {
                if ((t ^ d) / kWave != t / kWave) std::abort();
                nr[t] = tr[t] + tr[t ^ d];
                ni[t] = ti[t] + ti[t ^ d];
            }
            tr = nr;
            ti = ni;
        }
        for (uint32_t t = 0; t < T; t += fold) {
            pr[t / fold] = tr[t];
            pi[t / fold] = ti[t];
        }
        for (uint32_t t = 0; t < nblk; ++t) {
            int64_t br = 0, bi = 0;
            for (uint32_t k = 0; k < per; ++k) {
                if (t * per + k >= T) std::abort();
                br += pr[t * per + k];
                bi += pi[t * per + k];
            }
            bool zero;
            h[j0 + t] = (uint16_t)carrier_h(br, bi, &zero);
            r.stats[2] += zero;
        }
    }

    // ---- the flag pass: a workgroup per chunk, the ballot and the popcount parity of every wave
    const uint32_t est_m1 = carrier_state_est(c.state[0], c.init);
    const uint32_t hfirst = est_m1 & 0x7FFFu;
    int64_t steps = 0;
    for (uint64_t ch = 0; ch < g.nchunks; ++ch) {
        const uint64_t j_lo = ch * g.chunk, j_hi = g.nblocks < j_lo + g.chunk ? g.nblocks : j_lo + g.chunk;
        uint32_t carry = 0;
        for (uint64_t j0 = j_lo; j0 < j_hi; j0 += kCarrierFlagTurn) {
            uint32_t hv[kCarrierThreads][kCarrierFlagPer + 1] = {{0}}, pre[kCarrierThreads][kCarrierFlagPer] = {{0}}, run[kCarrierThreads] = {0};
            unsigned long long bal[kCarrierThreads / kWave] = {0};
            for (uint32_t t = 0; t < T; ++t) {
                const uint64_t jt = j0 + (uint64_t)kCarrierFlagPer * t;
                hv[t][0] = jt < j_hi ? (jt ? h[jt - 1] : hfirst) : 0u;
                for (uint32_t k = 0; k < kCarrierFlagPer; ++k) hv[t][k + 1] = jt + k < j_hi ? h[jt + k] : 0u;
                for (uint32_t k = 0; k < kCarrierFlagPer; ++k) {
                    if (jt + k < j_hi) {
                        const uint32_t f = carrier_flip(hv[t][k + 1], hv[t][k]);
                        steps += carrier_step(hv[t][k + 1], hv[t][k], f);
                        r.stats[1] += f;
                        run[t] ^= f;
                    }
                    pre[t][k] = run[t];
                }
                bal[t / kWave] |= (unsigned long long)run[t] << (t % kWave);
            }
            uint32_t total = 0;
            for (uint32_t t = 0; t < T; ++t) {
                const uint64_t jt = j0 + (uint64_t)kCarrierFlagPer * t;
                const uint32_t lane = t % kWave, wv = t / kWave;
                const uint32_t excl = (uint32_t)__builtin_popcountll(bal[wv] & ((1ull << lane) - 1ull)) & 1u;
                uint32_t before = 0;
                for (uint32_t k = 0; k < wv; ++k) before ^= (uint32_t)__builtin_popcountll(bal[k]) & 1u;
                const uint32_t base = excl ^ before ^ carry;
                for (uint32_t k = 0; k < kCarrierFlagPer; ++k)
                    if (jt + k < j_hi) e[jt + k] = (uint16_t)(hv[t][k + 1] | (pre[t][k] ^ base) << 15);
            }
            for (uint32_t k = 0; k < T / kWave; ++k) total ^= (uint32_t)__builtin_popcountll(bal[k]) & 1u;
            carry ^= total;
        }
        cpar[ch] = (uint8_t)carry;
    }
    r.stats[3] += (uint64_t)steps;

    // ---- the chain: 256 shares
    {
        const uint64_t share = carrier_chain_share(g.nchunks);
        uint8_t spar[kCarrierThreads], start[kCarrierThreads];
        auto lo_of = [&](uint32_t t) { return g.nchunks < t * share ? g.nchunks : t * share; };
        for (uint32_t t = 0; t < T; ++t) {
            const uint64_t lo = lo_of(t), hi = g.nchunks < lo + share ? g.nchunks : lo + share;
            uint32_t p = 0;
            for (uint64_t k = lo; k < hi; ++k) p ^= cpar[k];
            spar[t] = (uint8_t)p;
        }
        uint32_t b = est_m1 >> 15;
        for (uint32_t k = 0; k < T; ++k) {
            start[k] = (uint8_t)b;
            b ^= spar[k];
        }
        const uint32_t endb = b;
        for (uint32_t t = 0; t < T; ++t) {
            const uint64_t lo = lo_of(t), hi = g.nchunks < lo + share ? g.nchunks : lo + share;
            uint32_t bb = start[t];
            for (uint64_t k = lo; k < hi; ++k) {
                cstart[k] = (uint8_t)bb;
                bb ^= cpar[k];
            }
        }
        r.state[0] = g.nblocks ? kCarrierStarted | (e[g.nblocks - 1] & 0x7FFFu) | endb << 15 : c.state[0];
        r.state[1] = c.state[1] + g.nin;
        r.stats[0] += g.nblocks;
    }

    // ---- the est pass
    for (uint64_t ch = 0; ch < g.nchunks; ++ch) {
        const uint64_t j_lo = ch * g.chunk, j_hi = g.nblocks < j_lo + g.chunk ? g.nblocks : j_lo + g.chunk;
        for (uint64_t j = j_lo; j < j_hi; ++j) {
            e[j] = (uint16_t)(e[j] ^ (uint32_t)cstart[ch] << 15);
            r.phases[j] = e[j];
        }
    }

    // ---- the rotate pass: a thread's 8 decisions are one byte of the output
    uint8_t *bytes = reinterpret_cast<uint8_t *>(r.words.data());
    const uint64_t out_bytes = r.words.size() * 8;
    for (uint64_t tile = 0; tile < ntiles; ++tile) {
        const uint64_t j0 = tile * G, base = j0 * g.L;
        const uint32_t nblk = (uint32_t)(g.nblocks - j0 < G ? g.nblocks - j0 : G);
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t jb = t / L8;
            if (jb < nblk) {
                const uint32_t est = e[j0 + jb];
                const int cs = rom[carrier_adr_cos(est)], sn = rom[carrier_adr_sin(est)];
                const uint64_t p0 = base + 8 * t;
                const uint32_t nvalid = p0 >= g.nin ? 0u : (uint32_t)(g.nin - p0 < 8 ? g.nin - p0 : 8);
                int i[8], q[8];
                load8(c, g.nin, p0, t < G * L8, i, q);
                uint32_t byte = 0;
                for (uint32_t k = 0; k < 8; ++k) {
                    int io, qo;
                    carrier_rotate(i[k], q[k], cs, sn, io, qo);
                    byte |= (uint32_t)carrier_decide(io, c.threshold, c.strict != 0) << k;
                    if (k < nvalid) {
                        r.iq[2 * (p0 + k)] = (int16_t)io;
                        r.iq[2 * (p0 + k) + 1] = (int16_t)qo;
                        r.soft[p0 + k] = (int16_t)io;
                    }
                }
                if (p0 / 8 >= out_bytes) std::abort();
                bytes[p0 / 8] = (uint8_t)(byte & ((1u << nvalid) - 1u));
            }
            if (tile == ntiles - 1 && t < 8) {
                const uint64_t at = g.nblocks * L8 + t;
                if (at < out_bytes) bytes[at] = 0;
            }
        }
    }
    return r;
}

// the definition, one block after the other
Result serial(const Case &c) {
    Result r{};
    const uint64_t L = c.L, nall = c.in.size() / 2;
    const uint64_t nblocks = c.final ? (nall + L - 1) / L : nall / L, nin = nall < nblocks * L ? nall : nblocks * L;
    r.words.assign((nblocks * L + 63) / 64, 0);
    r.phases.resize(nblocks);
    r.iq.resize(2 * nin);
    r.soft.resize(nin);
    uint32_t est = (c.state[0] >> 63) ? (uint32_t)(c.state[0] & 0xFFFF) : c.init;
    int64_t steps = 0;
    for (uint64_t j = 0; j < nblocks; ++j) {
        const uint64_t lo = j * L, hi = nin < lo + L ? nin : lo + L;
        int64_t sr = 0, siq = 0;
        for (uint64_t n = lo; n < hi; ++n) {
            const int64_t i = c.in[2 * n], q = c.in[2 * n + 1];
            sr += i * i - q * q;
            siq += i * q;
        }
        const int64_t si = 2 * siq, ar = sr < 0 ? -sr : sr, ai = si < 0 ? -si : si, m = ar > ai ? ar : ai;
        int bl = 0;
        while (m >> bl) ++bl;
        const int s = bl > 15 ? bl - 15 : 0;
        uint32_t mag;
        int th;
        ddc_polar((int)(sr >> s), (int)(si >> s), mag, th);
        const uint32_t hj = ((uint32_t)th & 0xFFFF) >> 1, d = (hj - est) & 0xFFFF;
        const uint32_t next = (d < 16384 || d >= 49152) ? hj : (hj + 32768) & 0xFFFF;
        r.stats[0] += 1;
        r.stats[1] += (next >> 15) != (est >> 15);
        r.stats[2] += sr == 0 && si == 0;
        steps += (int16_t)(uint16_t)(next - est);
        est = next;
        r.phases[j] = (uint16_t)est;
        const int cs = rom[((est >> 6) + 256) & 1023], sn = rom[est >> 6];
        for (uint64_t n = lo; n < hi; ++n) {
            const int i = c.in[2 * n], q = c.in[2 * n + 1];
            int io = (i * cs + q * sn) >> 15, qo = (q * cs - i * sn) >> 15;
            io = io < -32768 ? -32768 : io > 32767 ? 32767 : io;
            qo = qo < -32768 ? -32768 : qo > 32767 ? 32767 : qo;
            r.iq[2 * n] = (int16_t)io;
            r.iq[2 * n + 1] = (int16_t)qo;
            r.soft[n] = (int16_t)io;
            const bool bit = c.strict ? io > c.threshold : io >= c.threshold;
            r.words[n >> 6] |= (uint64_t)bit << (n & 63);
        }
    }
    r.stats[3] = (uint64_t)steps;
    r.state[0] = nblocks ? kCarrierStarted | est : c.state[0];
    r.state[1] = c.state[1] + nin;
    return r;
}

// b_j = b_(j-1) XOR f_j against the serial rule, for every est_(-1) of a stride and h values on and around the ties
int scan_identity() {
    const uint32_t hs[] = {0, 1, 63, 64, 8191, 16383, 16384, 16385, 24575, 32766, 32767};
    int checked = 0;
    for (uint32_t est = 0; est < 65536; est += 37) {
        for (uint32_t hj : hs) {
            for (uint32_t dh : {0u, 1u, 16383u, 16384u, 16385u, 32767u}) {
                const uint32_t h2 = (hj + dh) & 0x7FFF;
                const uint32_t d = (h2 - est) & 0xFFFF;
                const uint32_t next = (d < 16384 || d >= 49152) ? h2 : (h2 + 32768) & 0xFFFF;
                const uint32_t f = carrier_flip(h2, est & 0x7FFF);
                if ((next >> 15) != ((est >> 15) ^ f)) return -1;
                if ((int)(int16_t)(uint16_t)(next - est) != carrier_step(h2, est & 0x7FFF, f)) return -1;
                ++checked;
            }
        }
    }
    return checked;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    load_rom(argv[3]);
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "w");
    if (!f || !o) return 2;
    if (scan_identity() <= 0) {
        std::fprintf(stderr, "the scan identity does not hold\n");
        return 1;
    }
    int ncases = 0;
    int64_t head[9];
    while (std::fread(head, 8, 9, f) == 9) {
        Case c;
        const uint64_t npairs = (uint64_t)head[0];
        c.L = (uint32_t)head[1], c.init = (uint32_t)head[2], c.threshold = (int32_t)head[3], c.strict = (uint32_t)head[4];
        c.chunk = (uint32_t)head[5], c.state[0] = (uint64_t)head[6], c.state[1] = (uint64_t)head[7], c.final = head[8] != 0;
        std::vector<int16_t> raw((2 * npairs + 3) / 4 * 4);
        if (!raw.empty() && std::fread(raw.data(), 2, raw.size(), f) != raw.size()) return 2;
        c.in.assign(raw.begin(), raw.begin() + 2 * npairs);
        const Result got = passes(c), want = serial(c);
        if (got.words != want.words || got.phases != want.phases || got.iq != want.iq || got.soft != want.soft ||
            std::memcmp(got.state, want.state, 16) || std::memcmp(got.stats, want.stats, 32)) {
            std::fprintf(stderr, "case %d: the passes differ from the serial loop\n", ncases);
            return 1;
        }
        std::fprintf(o, "%llu %llu %llu %llu %llu %lld\n", (unsigned long long)got.state[0], (unsigned long long)got.state[1],
                     (unsigned long long)got.stats[0], (unsigned long long)got.stats[1], (unsigned long long)got.stats[2], (long long)got.stats[3]);
        for (uint64_t w : got.words) std::fprintf(o, "%llx ", (unsigned long long)w);
        std::fprintf(o, "\n");
        for (uint16_t p : got.phases) std::fprintf(o, "%u ", p);
        std::fprintf(o, "\n");
        for (int16_t v : got.iq) std::fprintf(o, "%d ", v);
        std::fprintf(o, "\n");
        for (int16_t v : got.soft) std::fprintf(o, "%d ", v);
        std::fprintf(o, "\n");
        ++ncases;
    }
    std::fclose(f);
    std::fclose(o);
    std::printf("cases %d\n", ncases);
    return 0;
}
