// mlse_api.hip -- the extern "C" entry points of the Viterbi sequence detector (include/bbb.h, bbb_mlse_*).  Host logic only:
// the checks of bbb_mlse_cfg, the sizes of a call, the launch structure and the serial host model.
#include "capture.hpp"
#include "mlse_launch.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

using namespace bbb;

namespace {

// everything wrong with cfg that needs no device
int cfg_check(const bbb_mlse_cfg *c, MlseGeom *geom) {
    if (!c) return fail(BBB_EINVAL, "null mlse cfg");
    int rc = fir_cfg_check(&c->ff, false);
    if (rc) return rc;
    if (c->mem < 1 || c->mem > BBB_MLSE_MAX_MEM) return fail(BBB_EINVAL, "mem must be 1..4 (got " + std::to_string(c->mem) + ")");
    int64_t sum_g = 0;
    for (uint32_t i = 0; i <= c->mem; ++i) sum_g += std::llabs((long long)c->g[i]);
    if (sum_g > kMlseGBound) return fail(BBB_EINVAL, "sum |g| must be <= 2^20 (got " + std::to_string(sum_g) + ")");
    if (!mlse_geom(c->block_symbols, c->warmup_symbols, c->lookahead_symbols, *geom))
        return fail(BBB_EINVAL, "warmup_symbols and lookahead_symbols must be <= 128 and block + warmup + lookahead <= 512 (got " +
                                    std::to_string(geom->B) + ", " + std::to_string(geom->W) + ", " + std::to_string(geom->D) + ")");
    return BBB_OK;
}

// the sizes of a call, from sizes alone
int sizes(const bbb_mlse_cfg *c, const MlseGeom &geom, uint64_t nin, uint64_t first, int final, uint64_t *nsym, uint64_t *ndecided) {
    if (nin > kFirSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    *nsym = fir_nout(&c->ff, nin);
    if (first > kMlseSymbolLimit || *nsym > kMlseSymbolLimit - first) return fail(BBB_EINVAL, "first_symbol + nsym must be <= 2^58");
    *ndecided = mlse_ndecided(geom, first, *nsym, final != 0);
    return BBB_OK;
}

}  // namespace

extern "C" {

int bbb_mlse_plan(const bbb_mlse_cfg *cfg, uint64_t nin, uint64_t first_symbol, int final, uint64_t *nsym, uint64_t *ndecided,
                  uint64_t *nbefore_wanted) {
    MlseGeom geom;
    int rc = cfg_check(cfg, &geom);
    if (rc) return rc;
    uint64_t ns, nd;
    if ((rc = sizes(cfg, geom, nin, first_symbol, final, &ns, &nd))) return rc;
    if (nsym) *nsym = ns;
    if (ndecided) *ndecided = nd;
    if (nbefore_wanted) *nbefore_wanted = mlse_nbefore_wanted(geom, first_symbol, cfg->ff.decim, cfg->ff.ntaps, cfg->ff.phase);
    return BBB_OK;
}

// The definition, symbol by symbol and window by window, with nothing of mlse_common.hpp's core in it.
int bbb_mlse_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, uint64_t first_symbol, int final, const bbb_mlse_cfg *cfg,
                        uint64_t *bits_packed, uint64_t *ndecided_out) {
    MlseGeom geom;
    int rc = cfg_check(cfg, &geom);
    if (rc) return rc;
    uint64_t nsym, nd;
    if ((rc = sizes(cfg, geom, nin, first_symbol, final, &nsym, &nd))) return rc;
    if (nin && !in) return fail(BBB_EINVAL, "null in");
    if (nd && !bits_packed) return fail(BBB_EINVAL, "null bits_packed");
    if (ndecided_out) *ndecided_out = nd;
    const bbb_fir_cfg &ff = cfg->ff;
    const int L = (int)cfg->mem, NS = 1 << L;
    const int64_t B = geom.B, W = geom.W, D = geom.D, first = (int64_t)first_symbol, end = first + (int64_t)nsym;
    // y of the symbol k counted from the call's first (k < 0: history through nbefore, 0 beyond it)
    auto y_of = [&](int64_t k) {
        const int64_t n = (int64_t)ff.phase + k * (int64_t)ff.decim;
        int64_t acc = 0;
        for (uint32_t i = 0; i < ff.ntaps; ++i) {
            const int64_t j = n - (int64_t)i;
            if (j >= -(int64_t)nbefore && j < (int64_t)nin) acc += (int64_t)ff.taps[i] * in[j];
        }
        return std::min<int64_t>(std::max<int64_t>(acc >> ff.shift, -32768), 32767);
    };
    for (uint64_t w = 0; w < (nd + 63) / 64; ++w) bits_packed[w] = 0;
    if (!nd) return BBB_OK;
    std::vector<uint16_t> choice(kMlseMaxWindow);
    for (int64_t j = first / B; j * B < first + (int64_t)nd; ++j) {
        const int64_t lo = std::max<int64_t>(0, j * B - W), hi = std::min(end, (j + 1) * B + D);
        int64_t m[16], next[16];
        for (int h = 0; h < NS; ++h) m[h] = lo == 0 && h != (int)(cfg->init_state & (uint32_t)(NS - 1)) ? -(1ll << 62) : 0;
        for (int64_t K = lo; K < hi; ++K) {
            const int64_t y = y_of(K - first);
            uint16_t ch = 0;
            for (int hp = 0; hp < NS; ++hp) {
                int64_t cand[2];
                for (int c = 0; c < 2; ++c) {
                    const int h = (hp >> 1) | (c << (L - 1));
                    int64_t s = (hp & 1) ? cfg->g[0] : -(int64_t)cfg->g[0];
                    for (int i = 1; i <= L; ++i) s += (h >> (i - 1) & 1) ? cfg->g[i] : -(int64_t)cfg->g[i];
                    cand[c] = m[h] + 2 * y * s - s * s;
                }
                const int c = cand[1] > cand[0];
                next[hp] = cand[c];
                ch |= (uint16_t)(c << hp);
            }
            for (int h = 0; h < NS; ++h) m[h] = next[h];
            choice[(size_t)(K - lo)] = ch;
        }
        int s = 0;
        for (int h = 1; h < NS; ++h)
            if (m[h] > m[s]) s = h;
        for (int64_t K = hi - 1; K >= lo; --K) {
            if (K >= j * B && K < (j + 1) * B && K >= first && K < first + (int64_t)nd)
                bits_packed[(K - first) >> 6] |= (uint64_t)(s & 1) << ((K - first) & 63);
            s = (s >> 1) | ((choice[(size_t)(K - lo)] >> s & 1) << (L - 1));
        }
    }
    return BBB_OK;
}

int bbb_mlse_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_symbol, int final, const bbb_mlse_cfg *cfg,
                 uint64_t *bits_packed_dev, uint64_t *stats_dev, uint64_t *ndecided_out, int device, void *hip_stream) {
    MlseGeom geom;
    int rc = cfg_check(cfg, &geom);
    if (rc) return rc;
    uint64_t nsym, nd;
    if ((rc = sizes(cfg, geom, nin, first_symbol, final, &nsym, &nd))) return rc;
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (nd && !bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)bits_packed_dev & 7) || ((uintptr_t)stats_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    const bbb_fir_cfg &ff = cfg->ff;
    // the history the kernel reads: what the first window reaches, and no more than the caller says is there
    const uint32_t before = (uint32_t)std::min<uint64_t>(nbefore, mlse_nbefore_wanted(geom, first_symbol, ff.decim, ff.ntaps, ff.phase));
    const uint64_t bbytes = (nd + 63) / 64 * 8;
    if (overlap(in_dev - before, (nin + before) * 2, bits_packed_dev, bbytes)) return fail(BBB_EINVAL, "bits_packed_dev overlaps the samples");
    if (overlap(in_dev - before, (nin + before) * 2, stats_dev, stats_dev ? 16 : 0)) return fail(BBB_EINVAL, "stats_dev overlaps the samples");
    if (overlap(bits_packed_dev, bbytes, stats_dev, stats_dev ? 16 : 0)) return fail(BBB_EINVAL, "stats_dev overlaps bits_packed_dev");
    if (ndecided_out) *ndecided_out = nd;
    const hipStream_t st = (hipStream_t)hip_stream;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!nd) return BBB_OK;                        // nothing is decided: nothing is written
    MlseLaunch a{};
    a.in = in_dev;
    a.nin = nin;
    a.nbefore = before;
    a.ngroups = fir_pack_taps(&ff, a.taps);
    a.shift = ff.shift;
    a.decim = ff.decim;
    a.phase = ff.phase;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.mem = cfg->mem;
    for (uint32_t i = 0; i <= cfg->mem; ++i) a.g[i] = cfg->g[i];
    a.init_state = cfg->init_state & ((1u << cfg->mem) - 1);
    a.geom = geom;
    a.first = first_symbol;
    a.nsym = nsym;
    a.ndecided = nd;
    a.j0 = first_symbol / geom.B;
    a.nblocks = (first_symbol + nd - 1) / geom.B - a.j0 + 1;
    a.bits = bits_packed_dev;
    a.stats = stats_dev;
    // the words that two blocks share are ORed together
    BBB_HIP(hipMemsetAsync(bits_packed_dev, 0, bbytes, st));
    return mlse_launch(a, cus, st);
}

}  // extern "C"
