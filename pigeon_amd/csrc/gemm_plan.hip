// gemm_plan.hip -- host only, no kernels: which GEMM kernel runs which rows.  pg_gemm_launch, every GEMM of the encoder, checks its
// arguments, asks gemm_plan for a plan and makes at most two launcher calls.  Five bit-identical kernels take a GEMM:
//   PP6       gemm_pp6.hip   384 x 256 tiles, persistent
//   PP        gemm_pp.hip    256 x 256 tiles, persistent (variants 33 and 36: two rasters)
//   MID       gemm_mid.hip   128 x 128 tiles, one per block
//   TAIL      gemm_tail.hip  32 x 64 tiles, one per wave
//   ONE_TILE  gemm_bf16.hip  256 x 256 tiles, one per block (variant 8: the reference of the others)
// The plan is a pure function of the shape, the epilogue, the variant, the knobs and the CU count.  It is computed on every call and
// never cached: the knobs are baked into captured hipGraphs, which the tune epoch below invalidates; a plan cache would need the same.
#include "common.h"
#include "pigeon_internal.h"

#include "gemm_epi.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>

// ================================================================================================================ knobs
// Every knob is read once from its environment variable (or set by its pg_tune_* call) and then cached.  Every pg_tune_gemm_* call
// bumps the epoch: the knobs are baked into captured launches, so a hipGraph of an older epoch is re-captured (vit.hip).
#ifndef PG_DEFAULT_GEMM_STAGGER
#define PG_DEFAULT_GEMM_STAGGER 0.0f
#endif
// Tail split (gemm_tail.hip).  ROWS: most rows handed to a small-tile kernel instead of giving them a (mostly idle) last round of the
// persistent kernels; 768 = two 384-row panels.  The split is used only where it measured positive on the 512-image step
// (profiles/r02/gemm_tail.txt): K >= 2048 (fc2: a 120 us round saved for a 43 us tail launch, +0.4 % end to end) or N >= 4096 (fc1,
// +0.1 %); for out-projection and QKV the tail launch costs what the half-idle round did (-0.2 % with all four).
#define PG_DEFAULT_GEMM_TAIL_ROWS 768
#define PG_DEFAULT_GEMM_TAIL_MIN_K 2048
#define PG_DEFAULT_GEMM_TAIL_MIN_N 4096
// EPI_RESID_STAT on the 384 x 256 kernel (round 3): bit 0 = long-K GEMMs (fc2, K >= 2048), bit 1 = short-K ones (out-projection).
// Results are bit-identical either way; this only selects the tile shape.  Env PIGEON_GEMM_RESID6 (A/B).  Measured on the 512-image
// step (profiles/r03/pp6_resid_stat_ab.txt): fc2 2.224 -> 2.152 ms (-3.2 %; W is re-streamed through every XCD's L2 12 instead of 18
// times), out-projection 0.90 -> 0.976 ms (its epilogue is 43 % of a tile, first build): the default takes fc2 only, +0.9 % end to end.
#ifndef PG_DEFAULT_GEMM_RESID6
#define PG_DEFAULT_GEMM_RESID6 1
#endif
#define PG_ROUTE_MAX_ROWS 40000   // the routing model is fitted up to 64 images (36 928 token rows); above that a variant means its kernel
#ifndef PG_EXACT_MID_US_KT
#define PG_EXACT_MID_US_KT 0.6
#endif

static unsigned long long g_tune_epoch = 1;
unsigned long long pg_tune_epoch() { return g_tune_epoch; }

// the one reader of the knobs' environment variables: atoi for integers, atof for reals, the raw string otherwise; dflt when unset
template <typename T>
static T env_knob(const char* name, T dflt) {
    const char* e = getenv(name);
    if (!e) return dflt;
    if constexpr (std::is_integral<T>::value) return (T)atoi(e);
    else if constexpr (std::is_floating_point<T>::value) return (T)atof(e);
    else return e;
}

int pg_default_gemm_variant() {
    static int v = -1;
    if (v < 0) {
        // 56: persistent ping-pong kernel with 384 x 256 tiles for the QKV / fc1 GEMMs (gemm_pp6.hip), 256 x 256 (variant 36:
        // 8x4 super-tile raster, gemm_pp.hip) for everything else
        v = env_knob("PIGEON_GEMM_VARIANT", (int)PG_GEMM_V_PP6);
        if (v <= 0) v = PG_GEMM_V_PP6;
    }
    return v;
}
static int block_cap() {
    static int v = -1;
    if (v < 0) { v = env_knob("PIGEON_GEMM_BLOCKS", 0); if (v < 0) v = 0; }
    return v;
}
static int route_max_rows() {     // (env PIGEON_GEMM_ROUTE_MAX_ROWS: experiments beyond the fitted range)
    static int v = -1;
    if (v < 0) { v = env_knob("PIGEON_GEMM_ROUTE_MAX_ROWS", PG_ROUTE_MAX_ROWS); if (v < 0) v = 0; }
    return v;
}
static bool resid6_enabled(int K) {
    static int mask = -1;
    if (mask < 0) { mask = env_knob("PIGEON_GEMM_RESID6", PG_DEFAULT_GEMM_RESID6); if (mask < 0) mask = 0; }
    return (mask & (K >= 2048 ? 1 : 2)) != 0;
}
static double precise_mid_us_kt() {     // microseconds per K tile of a gemm_mid round in the exact tier's routing (env PIGEON_EXACT_MID_US: A/B)
    static double v = -1.0;
    if (v < 0.0) { v = env_knob("PIGEON_EXACT_MID_US", PG_EXACT_MID_US_KT); if (!(v > 0.0)) v = PG_EXACT_MID_US_KT; }
    return v;
}

static int g_raster_gn = -2;
int pg_gemm_raster_gn() {
    if (g_raster_gn == -2) { g_raster_gn = env_knob("PIGEON_GEMM_RASTER_GN", 0); if (g_raster_gn < -1) g_raster_gn = 0; }
    return g_raster_gn;
}
extern "C" int pg_tune_gemm_raster(int gn) {
    if (gn < -1 || gn > 64) { pg_set_error("tune_gemm_raster: gn must be -1 (all N tiles), 0 (default) or 1..64"); return PG_EINVAL; }
    g_raster_gn = gn; ++g_tune_epoch;
    return PG_OK;
}

static int g_tail_rows = -1, g_tail_min_k = -1, g_tail_min_n = -1;
static int env_count(const char* name, int dflt) { const int v = env_knob(name, dflt); return v < 0 ? 0 : v; }
static int tail_rows() { if (g_tail_rows < 0) g_tail_rows = env_count("PIGEON_GEMM_TAIL_ROWS", PG_DEFAULT_GEMM_TAIL_ROWS); return g_tail_rows; }
static int tail_min_k() { if (g_tail_min_k < 0) g_tail_min_k = env_count("PIGEON_GEMM_TAIL_MIN_K", PG_DEFAULT_GEMM_TAIL_MIN_K); return g_tail_min_k; }
static int tail_min_n() { if (g_tail_min_n < 0) g_tail_min_n = env_count("PIGEON_GEMM_TAIL_MIN_N", PG_DEFAULT_GEMM_TAIL_MIN_N); return g_tail_min_n; }
extern "C" int pg_tune_gemm_tail_rows(int rows) {
    if (rows < 0 || rows > (1 << 20)) { pg_set_error("tune_gemm_tail_rows: rows must be in [0, 2^20]"); return PG_EINVAL; }
    g_tail_rows = rows; ++g_tune_epoch;
    return PG_OK;
}
extern "C" int pg_tune_gemm_tail_shape(int min_k, int min_n) {
    if (min_k < 0 || min_n < 0) { pg_set_error("tune_gemm_tail_shape: negative threshold"); return PG_EINVAL; }
    g_tail_min_k = min_k; g_tail_min_n = min_n; ++g_tune_epoch;
    return PG_OK;
}

static int g_gemm_mid = -1;
static bool mid_on() {
    if (g_gemm_mid < 0) { const char* e = env_knob<const char*>("PIGEON_GEMM_MID", "1"); g_gemm_mid = e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1); }
    return g_gemm_mid != 0;
}
static bool route_pp256() { return mid_on() && g_gemm_mid != 2; }   // 2 (A/B arm): gemm_mid.hip is the only alternative
extern "C" int pg_tune_gemm_mid(int on) {
    g_gemm_mid = on == 2 ? 2 : (on ? 1 : 0); ++g_tune_epoch;
    return PG_OK;
}

static float g_stagger = -1.f;
static float stagger_fraction() {
    if (g_stagger < 0.f) {
        g_stagger = env_knob("PIGEON_GEMM_STAGGER", PG_DEFAULT_GEMM_STAGGER);
        if (!(g_stagger >= 0.f && g_stagger <= 4.f)) g_stagger = 0.f;
    }
    return g_stagger;
}
extern "C" int pg_tune_gemm_stagger(float fraction) {
    if (!(fraction >= 0.f && fraction <= 4.f)) { pg_set_error("tune_gemm_stagger: fraction must be in [0, 4]"); return PG_EINVAL; }
    g_stagger = fraction; ++g_tune_epoch;
    return PG_OK;
}

// ================================================================================================================ CU count
static int num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}
int pg_gemm_grid_cus() {
    const int ncu = num_cus(), cap = block_cap();
    return cap > 0 && cap < ncu ? cap : ncu;          // tuning: share the chip between streams
}

// ================================================================================================================ cost models
// Four models of the same kernels, each fitted on its own: their constants differ on purpose and routing depends on every one.

// (1) Small and middle batches (round 6): modelled time (us) of one launch on `ncu` CUs through kernel PP6, PP or MID, for batches
// of up to ~64 images.  A persistent launch is a sequence of rounds; a round's tile period grows with the share f of the CUs it keeps
// busy (the power cap: 2.4 GHz on an idle chip, ~1.7 GHz on a full one), c(f) = ci + (cf - ci) f^2 microseconds per 64-wide K tile,
// plus an epilogue the first round pays in full (e1) and the later ones partly (e2: the next tile's operands are in flight under it).
// Fitted to profiles/r06/gemm_three_sweep.txt (the model's four GEMM shapes x 1 .. 64 images x the three kernels): the pick is the
// measured best, or within 0.4 % of it, in all 36 cells.  (Second session: gemm_mid's two constants refitted to
// gemm_three_sweep_producer.txt -- its producer wave; the pick is within 9 % of the best in every cell of the first file and of the
// two residual shapes of the second, tests/test_host_cpu.py.)
struct PersistentFit { double ci, cf, e1_resid, e1_gelu, e1_other, e2; };
constexpr PersistentFit SMALL_PP6 = {1.6, 3.0, 7.0, 9.0, 6.0, 3.0};       // 384 x 256
constexpr PersistentFit SMALL_PP = {1.1, 1.8, 12.0, 9.0, 7.0, 6.0};       // 256 x 256
// 128 x 128 through the 3-stage ring with the producer wave (0.41 measured on fc2's 64 K tiles, profiles/r06/
// gemm_three_sweep_producer.txt; 0.58 - 0.62 while the MFMA waves issued their own DMAs: gemm_mid_sweep.txt)
constexpr double SMALL_MID_US_KT = 0.44;
constexpr double SMALL_MID_EPI_RESID = 8.0, SMALL_MID_EPI = 5.5;          // gemm_mid's epilogue per round, same fit
// the 256 x 256 kernel has to win by a margin: where the model calls it level with the 384 x 256 kernel (64 images) or with
// gemm_mid (2 and 8 images) the encoder measured 1 - 3 % SLOWER with it in place (profiles/r06/latency_route_ab.txt: a
// launch in a forward is not a launch in a loop of its own); where it wins by more, the encoder gains 3 - 9 %
constexpr double SMALL_PP_MARGIN = 0.90;

static double gemm_model_us(int kernel, int M, int N, int K, int epi, int ncu) {
    const bool resid = epi == EPI_RESID || epi == EPI_RESID_STAT;
    const bool gelu = epi == EPI_GELU || epi == EPI_GELU_LN;
    const double kt = K / 64;
    if (kernel == PG_GK_MID) {
        const int64_t tiles = (int64_t)((M + 127) / 128) * (N / 128);
        return (double)((tiles + ncu - 1) / ncu) * (kt * SMALL_MID_US_KT + (resid ? SMALL_MID_EPI_RESID : SMALL_MID_EPI));
    }
    const PersistentFit& c = kernel == PG_GK_PP6 ? SMALL_PP6 : SMALL_PP;
    const int bm = kernel == PG_GK_PP6 ? 384 : 256;
    const double e1 = resid ? c.e1_resid : (gelu ? c.e1_gelu : c.e1_other);
    const int64_t tiles = (int64_t)((M + bm - 1) / bm) * (N / 256);
    const int64_t full = tiles / ncu;
    const double f = (double)(tiles % ncu) / (double)ncu;
    double t = 0.0;
    if (full > 0) t += kt * c.cf + e1 + (double)(full - 1) * (kt * c.cf + c.e2);
    if (f > 0.0) t += kt * (c.ci + (c.cf - c.ci) * f * f) + (full > 0 ? c.e2 : e1);
    return t;
}

// (2) Tail split: the round the cut removes against the small-tile launch that takes its rows.  gemm_tail.hip needs ~36 us for the
// benchmark batch's 512 rows whatever the shape (profiles/r02/gemm_tail.txt, profiles/r06/step_kernel_stats.csv); gemm_mid.hip does a
// K = 1024 tail in 15 - 19 us (profiles/r06/gemm_mid_sweep.txt, the n = 1 column) and a K = 4096 one in 44.
constexpr double TAIL_US = 36.0;                                          // gemm_tail.hip on a <= 768-row tail, either shape
constexpr double ROUND_US_KT_PP6 = 1.75, ROUND_US_KT_PP = 1.25;           // a round on a mostly idle chip (2.4 GHz): a lower bound on a busy one
constexpr double ROUND_EPI_PP6_RESID = 14.0, ROUND_EPI_PP6 = 9.0;         // ... plus its epilogue (profiles/r06/tail_mid_ab.txt)
constexpr double ROUND_EPI_PP_RESID = 20.0, ROUND_EPI_PP = 8.0;
constexpr double TAIL_MID_EPI_RESID = 6.0, TAIL_MID_EPI = 5.0, TAIL_MID_LAUNCH_US = 3.0;   // gemm_mid on the tail: epilogue per round, a launch

// (3) XCD stagger (gemm_device.h): total spread = fraction x estimated tile period.  Tile periods measured on MI355X (profiles/r02):
// 256 x 256 tiles 25 us + 1.63 us per 64-wide K tile (fp32 residual epilogues; 10 us otherwise), 384 x 256 tiles 8 us (+4 us with
// the GELU) + 2.44 us per K tile.
constexpr float STAGGER_PP6_EPI = 8.f, STAGGER_PP6_EPI_GELU = 12.f, STAGGER_PP6_US_KT = 2.44f;
constexpr float STAGGER_PP_EPI = 10.f, STAGGER_PP_EPI_RESID = 25.f, STAGGER_PP_US_KT = 1.63f;
constexpr float TICKS_PER_US = 100.f;                                     // s_memrealtime: 100 MHz

// (4) The exact tier (vit.hip precise_gemm): rounds(S) x (K tiles per part x 1.7 us + epilogue) + the sum pass (S + 1 or S + 2
// streams of M x N floats at ~4 TB/s).  Measured on MI355X (profiles/r05, 8 images): out-projection 107 -> 54 us, fc2 351 -> 158 us
// with S = 3 / 6; QKV and fc1 (216 / 288 tiles of 48 K tiles) gain nothing from a split at that size and lose at larger ones, which
// the model reproduces.  gemm_mid's K tile: PG_EXACT_MID_US_KT (0.6; profiles/r06 A/B: 0.5 / 0.44 were slower).
constexpr double EXACT_US_KT = 1.7;
constexpr double EXACT_EPI_RESID_WHOLE = 25.0, EXACT_EPI = 12.0;          // S = 1 with the residual read-modify-write / otherwise
constexpr double EXACT_SUM_LAUNCH_US = 4.0, EXACT_SUM_BYTES_PER_US = 4.0e6;
constexpr double EXACT_MID_EPI_RESID = 6.0, EXACT_MID_EPI = 5.0;

// How many K-parts for one GEMM of the exact mode: the S (out of `cand`) with the smallest modelled time.  A pure function of the
// shape: the same batch size always takes the same path (results differ between S only in fp32 summation order, ~1e-7 relative, two
// orders below the exact tier's own floor).  Quirk kept: the exact tier's models use the uncapped CU count, PIGEON_GEMM_BLOCKS does
// not reach them (the small-batch route and the tail split use the capped one).
static int precise_parts(int M, int N, int Ktot, bool resid, const int* cand, int ncand, double* best_us_out) {
    const double ncu = (double)num_cus();
    const double tiles = (double)((M + 255) / 256) * (N / 256);
    int best = 1; double best_us = 1e30;
    for (int i = 0; i < ncand; ++i) {
        const int S = cand[i];
        if (Ktot % S || (Ktot / S) % 128) continue;
        const double rounds = ceil(S * tiles / ncu);
        const double epi = (S == 1 && resid) ? EXACT_EPI_RESID_WHOLE : EXACT_EPI;
        double us = rounds * ((Ktot / S / 64) * EXACT_US_KT + epi);
        if (S > 1) us += EXACT_SUM_LAUNCH_US + (double)(S + (resid ? 2 : 1)) * M * N * 4.0 / EXACT_SUM_BYTES_PER_US;
        if (us < best_us) { best_us = us; best = S; }
    }
    if (best_us_out) *best_us_out = best_us;
    return best;
}
// Round 6: a handful of images (a settled-at-once exact pass: serving, certain_forward) -- the 128 x 128 one-tile-per-block kernel
// (gemm_mid.hip) keeps the whole K' in one chain like S = 1 and still fills the chip.  Bit-identical to the S = 1 persistent launch.
int pg_gemm_precise_route(int M, int N, int Ktot, bool resid, const int* cand, int ncand) {
    double parts_us = 0.0;
    const int S = precise_parts(M, N, Ktot, resid, cand, ncand, &parts_us);
    if (mid_on() && N % 128 == 0) {
        const double rounds_m = ceil((double)((M + 127) / 128) * (N / 128) / (double)num_cus());
        const double mid_us = rounds_m * ((Ktot / 64) * precise_mid_us_kt() + (resid ? EXACT_MID_EPI_RESID : EXACT_MID_EPI));
        if (mid_us < parts_us) return 0;
    }
    return S;
}

// ================================================================================================================ the plan
struct GemmPlan {
    int kernel;          // PgGemmKernel of the main launch
    int variant;         // passed to it: the raster / schedule variant for PP, the one-tile variant for ONE_TILE
    int rows;            // the main launch takes rows [0, rows)
    int rest;            // kernel of rows [rows, M): PG_GK_NONE, PG_GK_MID or PG_GK_TAIL
    int stagger_ticks;   // GemmArgs::xcd_stagger_ticks of both launches
};

static bool is_pp_variant(int v) { return v == 33 || v == PG_GEMM_V_PP; }
static bool use_pp6(int variant, int epi, int N, int K) {
    return variant == PG_GEMM_V_PP6 && pg_gemm_pp6_supported(epi, N, K) && (epi != EPI_RESID_STAT || resid6_enabled(K));
}

// Small and middle batches (round 6).  The product variant (56) means "384 x 256 tiles where they exist, 256 x 256 elsewhere", chosen
// for the 512-image step, where a launch is 12 - 50 rounds.  Up to ~64 images a launch is 1 - 7 rounds and what decides is how the row
// panels of a tile shape fill whole rounds of the CUs: one panorama (2308 rows) is 7 panels of 384 or 10 of 256 or 19 of 128; 16
// images leave the 384-row kernel a second round with 44 of 256 CUs busy.  pg_tune_gemm_mid(0) / PIGEON_GEMM_MID=0: the variant's own
// kernel, always.  Measured (profiles/r06/gemm_three_sweep.txt, latency_route.txt): 16 images QKV 79.7 -> 64.6 us, fc2 123.5 -> 94.6;
// one panorama fc1 38.7 -> 31.7.  Returns the pick among `own` (PP6 or PP), PP and MID.
static int small_batch_route(int own, int epi, int M, int N, int K) {
    if (!(mid_on() && M <= route_max_rows() && epi != EPI_PATCH && epi >= EPI_QKV && epi <= EPI_GELU_LN)) return own;
    const int ncu = pg_gemm_grid_cus();
    const double t_own = gemm_model_us(own, M, N, K, epi, ncu);
    const double t_pp = (own == PG_GK_PP6 && route_pp256()) ? gemm_model_us(PG_GK_PP, M, N, K, epi, ncu) : 1e30;
    const double t_mid = pg_gemm_mid_supported(epi, N, K) ? gemm_model_us(PG_GK_MID, M, N, K, epi, ncu) : 1e30;
    if (t_pp < SMALL_PP_MARGIN * t_own && t_pp < SMALL_PP_MARGIN * t_mid) return PG_GK_PP;
    return t_mid < t_own ? PG_GK_MID : own;
}

// Tail split: if the tiles do not fill the persistent kernel's last round and the rows beyond the last whole round are few, the
// persistent kernel gets the rows that make whole rounds and a small-tile kernel the rest.  WHERE to cut is round 2's measurement (the
// MIN_K / MIN_N knobs: fc2 and fc1; for out-projection and QKV the extra launch costs what the 8-tile last round did -- measured again
// in round 6 with the cheaper tail kernel, profiles/r06/tail_mid_ab.txt: still nothing end to end).  WHICH kernel takes the tail is
// cost model (2): fc1's tail goes through gemm_mid (the fc1 launch pair 2.257 -> 2.237 ms, 0.4347 -> 0.4384 of the MFMA peak on one
// box), fc2's through gemm_tail.  Sets p.rows / p.rest and returns true where it cuts.
static bool tail_split(int own, int epi, int M, int N, int K, GemmPlan& p) {
    const int tail_max = tail_rows();
    if (tail_max <= 0) return false;
    const bool six = own == PG_GK_PP6;
    const int bm = six ? 384 : 256;
    const int ncu = pg_gemm_grid_cus();
    const int tilesN = N / 256;
    const int64_t ntiles = (int64_t)((M + bm - 1) / bm) * tilesN;
    const int64_t rounds = ntiles / ncu;
    if (rounds < 1 || ntiles % ncu == 0) return false;
    const int64_t m_main = (rounds * ncu / tilesN) * bm;                 // row panels that fit into `rounds` whole rounds
    if (!(m_main > 0 && m_main < M && M - m_main <= tail_max)) return false;
    const bool resid = epi == EPI_RESID || epi == EPI_RESID_STAT;
    const double kt = K / 64;
    const double t_round = six ? kt * ROUND_US_KT_PP6 + (resid ? ROUND_EPI_PP6_RESID : ROUND_EPI_PP6)
                               : kt * ROUND_US_KT_PP + (resid ? ROUND_EPI_PP_RESID : ROUND_EPI_PP);
    const int64_t tiles_m = (int64_t)((M - m_main + 127) / 128) * (N / 128);
    const double t_mid = (double)((tiles_m + ncu - 1) / ncu) * (kt * SMALL_MID_US_KT + (resid ? TAIL_MID_EPI_RESID : TAIL_MID_EPI)) + TAIL_MID_LAUNCH_US;
    const bool cut = K >= tail_min_k() || N >= tail_min_n();
    const bool by_mid = cut && mid_on() && pg_gemm_mid_supported(epi, N, K) && t_mid < TAIL_US && t_mid < t_round;
    const bool by_tail = cut && !by_mid && pg_gemm_tail_supported(epi, N, K);
    if (!by_mid && !by_tail) return false;
    p.rows = (int)m_main;
    p.rest = by_mid ? PG_GK_MID : PG_GK_TAIL;
    return true;
}

// Quirk kept: the period is that of the variant's OWN kernel (use_pp6), also where the small-batch route then launches another one.
static int stagger_ticks(bool six, int epi, int M, int K) {
    const float f = stagger_fraction();
    if (!(f > 0.f && M >= 256 * 64)) return 0;
    const float period_us = six ? ((epi == EPI_GELU || epi == EPI_GELU_LN ? STAGGER_PP6_EPI_GELU : STAGGER_PP6_EPI) + STAGGER_PP6_US_KT * (K / 64))
                                : ((epi == EPI_RESID || epi == EPI_RESID_STAT ? STAGGER_PP_EPI_RESID : STAGGER_PP_EPI) + STAGGER_PP_US_KT * (K / 64));
    return (int)(f * period_us * TICKS_PER_US);
}

// variant 0 = the default.  PG_EINVAL (with the message) where no kernel of this build takes the call.
static int gemm_plan(int variant, int epi, int M, int N, int K, GemmPlan& p) {
    if (epi < EPI_QKV || epi > EPI_GELU_X3) { pg_set_error("gemm: bad epilogue %d", epi); return PG_EINVAL; }
    if (variant == 0) variant = pg_default_gemm_variant();
    const bool six = use_pp6(variant, epi, N, K);
    const bool pp = !six && (variant == PG_GEMM_V_PP6 || is_pp_variant(variant)) && N % 256 == 0 && K % 128 == 0;
    const int own = six ? PG_GK_PP6 : PG_GK_PP;
    // the PP launch of variant 56 is the product raster 36
    const int pp_variant = variant == PG_GEMM_V_PP6 ? PG_GEMM_V_PP : variant;
    p = GemmPlan{own, pp_variant, M, PG_GK_NONE, stagger_ticks(six, epi, M, K)};
    if (variant == PG_GEMM_V_MID || variant == PG_GEMM_V_TAIL) {          // the whole problem through one small-tile kernel (tests, tools)
        const bool mid = variant == PG_GEMM_V_MID;
        if (!(mid ? pg_gemm_mid_supported(epi, N, K) : pg_gemm_tail_supported(epi, N, K))) {
            pg_set_error("gemm: variant %d (%s) does not support epi=%d N=%d K=%d", variant, mid ? "gemm_mid" : "gemm_tail", epi, N, K);
            return PG_EINVAL;
        }
        p.kernel = mid ? PG_GK_MID : PG_GK_TAIL;
        return PG_OK;
    }
    if (six || pp) {
        // Quirk kept: the small-batch route's PP launch is always raster variant 36, whatever the caller's variant
        const int kind = small_batch_route(own, epi, M, N, K);
        if (kind != own) {
            p.kernel = kind;
            p.variant = PG_GEMM_V_PP;
            return PG_OK;
        }
        // Quirk kept: the tail split runs only where the small-batch route kept the variant's own kernel
        tail_split(own, epi, M, N, K, p);
        return PG_OK;
    }
    // the one-tile-per-block kernel: variant 8 for the persistent variants on shapes they do not take, else the caller's variant
    if (epi >= EPI_RESID_STAT) { pg_set_error("gemm: epilogue %d exists only in the persistent kernels (variants 33, 36, 56, N %% 256 == 0, K %% 128 == 0)", epi); return PG_EINVAL; }
    p.kernel = PG_GK_ONE_TILE;
    p.variant = (variant == PG_GEMM_V_PP6 || is_pp_variant(variant)) ? PG_GEMM_V_ONE_TILE : variant;
    const int bn = pg_gemm_one_tile_bn(p.variant);
    if (bn == 0) {
        pg_set_error("gemm: variant %d does not exist (variants: 8, 33, 36, 56, 70, 71)", p.variant);
        return PG_EINVAL;
    }
    if (N % bn != 0 || K % BK != 0) { pg_set_error("gemm: N %% %d or K %% 64 != 0 (N=%d K=%d)", bn, N, K); return PG_EINVAL; }
    return PG_OK;
}

// (exported for the host-logic tests and tools: no launch, no device work)
extern "C" int pg_gemm_plan(int variant, int epi, int M, int N, int K, int* kernel, int* rows_main, int* rest) {
    if (!kernel || !rows_main || !rest || M <= 0 || N <= 0 || K <= 0) { pg_set_error("gemm_plan: bad argument"); return PG_EINVAL; }
    GemmPlan p;
    const int rc = gemm_plan(variant, epi, M, N, K, p);
    if (rc != PG_OK) return rc;
    *kernel = p.kernel; *rows_main = p.rows; *rest = p.rest;
    return PG_OK;
}

#ifdef PIGEON_PROBES
static void* g_dbg_ts = nullptr;
// probe build: arm (buf != null) / disarm the PG_TS time stamps of the persistent kernels; buf = 2 * 16 * 8 * 12 uint64 on the device
extern "C" int pg_dbg_timestamps(void* buf) { g_dbg_ts = buf; return PG_OK; }
#endif

static int launch_one(int kernel, int variant, int dtype, const GemmArgs& g, int epi, int m_begin, hipStream_t s) {
    switch (kernel) {
        case PG_GK_PP6: return pg_gemm_pp6_launch(dtype, g, epi, s);
        case PG_GK_PP: return pg_gemm_pp_launch(dtype, g, epi, variant, s);
        case PG_GK_MID: return pg_gemm_mid_launch(dtype, g, epi, s, m_begin);
        case PG_GK_TAIL: return pg_gemm_tail_launch(dtype, g, epi, m_begin, s);
        default: return pg_gemm_one_tile_launch(dtype, g, epi, variant, s);
    }
}

int pg_gemm_launch(int dtype, const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldc,
                   int M, int N, int K, int epi, float qscale, int qcols, const float* aux, int variant,
                   hipStream_t s, const PgGemmExtra* extra) {
    if (M <= 0) return PG_OK;
    GemmArgs g;
    g.A = (const uint16_t*)A; g.lda = lda; g.W = (const uint16_t*)W; g.ldw = ldw > 0 ? ldw : K; g.bias = bias; g.out = out; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.qscale = qscale; g.qcols = qcols; g.aux = aux;
    g.tilesM = 0; g.tilesN = 0; g.ntiles = 0; g.part_tiles = 0; g.gn = 0; g.stagger = 0; g.xcd_stagger_ticks = 0;
    if (extra) g.ex = *extra;
    if (g.ex.parts > 1) {                                    // several products in one launch: 256 x 256 persistent kernel, EPI_F32 only
        if (epi != EPI_F32 || N % 256 != 0 || K % 128 != 0) { pg_set_error("gemm: parts > 1 needs EPI_F32, N %% 256 == 0, K %% 128 == 0"); return PG_EINVAL; }
        return pg_gemm_pp_launch(dtype, g, epi, PG_GEMM_V_PP, s);
    }
    if ((epi == EPI_GELU || epi == EPI_RESID || epi >= EPI_RESID_STAT) && !bias) { pg_set_error("gemm: epilogue %d needs a bias", epi); return PG_EINVAL; }
    if (epi == EPI_RESID_STAT && (!g.ex.x16 || !g.ex.statpart || g.ex.ldx != ldc)) { pg_set_error("gemm: EPI_RESID_STAT needs x16 / statpart and ldx == ldc"); return PG_EINVAL; }
    if (epi_is_ln(epi) && (!g.ex.colsum || !g.ex.rowstat)) { pg_set_error("gemm: LN epilogue needs colsum / rowstat"); return PG_EINVAL; }
    if (epi == EPI_PATCH && !aux) { pg_set_error("gemm: patch epilogue needs aux"); return PG_EINVAL; }
    if (epi == EPI_GELU_X3 && (ldc != 3 * (int64_t)N || dtype != PG_DTYPE_F16 || N % 256 != 0 || K % 128 != 0)) {
        pg_set_error("gemm: EPI_GELU_X3 writes the fp16 triple [M][3N]: ldc == 3 N, fp16 operands, N %% 256 == 0, K %% 128 == 0 (ldc=%lld N=%d K=%d)",
                     (long long)ldc, N, K);
        return PG_EINVAL;
    }
    if ((lda % 8) || (ldc % 8) || (qcols % 8) || (g.ldw % 8) || g.ldw < K) { pg_set_error("gemm: lda/ldw/ldc/qcols must be multiples of 8, ldw >= K"); return PG_EINVAL; }
    GemmPlan p;
    const int rc = gemm_plan(variant, epi, M, N, K, p);
    if (rc != PG_OK) return rc;
    g.xcd_stagger_ticks = p.stagger_ticks;
    if (g.ex.stat_rows <= 0) g.ex.stat_rows = M;
#ifdef PIGEON_PROBES
    if (g_dbg_ts && epi != EPI_PATCH) { g.aux = (const float*)g_dbg_ts; g.stagger = -7; }
#endif
    // all five kernels produce the same bits for a row: the plan changes timing only
    GemmArgs gm = g;
    gm.M = p.rows;
    const int rc_main = launch_one(p.kernel, p.variant, dtype, gm, epi, 0, s);
    if (rc_main != PG_OK || p.rest == PG_GK_NONE) return rc_main;
    return launch_one(p.rest, 0, dtype, g, epi, p.rows, s);
}
