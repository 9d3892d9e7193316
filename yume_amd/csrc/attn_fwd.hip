// attn_fwd.hip — exact-softmax attention forward for head_dim 128, bf16 in / fp32 accumulate / bf16 out (gfx950): the C-ABI entry points
// (yume_attn_fwd, yume_attn_fwd_ws, yume_attn_fwd_kw, yume_attn_fwd_band, yume_attn_fwd_fband, yume_attn_fwd_seg, yume_attn_fwd_batch, yume_attn_workspace_bytes,
// yume_attn_batch_workspace_bytes) and the dispatcher behind them:
// validate -> choose -> launch.
//
// Seven kernels compute the same function (choose() picks; the tests compare them). Each lives in a file of its own with its design comment:
//   attn_fwd_kernel_v8    attn_fwd8.hip       persistent workgroups over one continuous K / V^T stream (self-attention; needs pre-scaled Q,
//                                             padded K / V^T and a counter set)
//   attn_fwd_kernel_v7    attn_fwd7.hip       4 waves x 64 queries, one wave per SIMD (self-attention, Lk >= 1536, where v8 does not apply)
//   attn_fwd_kernel_v4    attn_fwd_v4.hpp     8 waves, 256 queries per workgroup, software-pipelined across key tiles (variant 4 only)
//   attn_fwd_kernel_v2    attn_fwd_v2.hpp     4 waves, 128 queries, two workgroups per CU, K / V^T tiles by LDS-DMA (cross-attention, short
//                                             launches; <true>: a WEIGHTED LAST KEY, yume_attn_fwd_kw, any Lk)
//   attn_fwd_kernel       attn_fwd_v1.hpp     as v2 with register-staged tiles (the first version; kept as an independent cross-check)
//   attn_cross_rk_kernel  attn_cross_rk.hpp   448 < Lk <= 512: K and V^T resident in a workgroup's registers
//   attn_short_kernel     attn_short.hpp      Lk <= 128: a head's K and V^T resident in one wave's registers (takes the weighted last key)
// yume_attn_fwd_seg (several independent segments in one launch) has the segmented forms of the last two of its own: attn_seg.hpp.
// yume_attn_fwd_batch (several stacked self-attention problems of one shape) has attn_fwd_kernel_v8's: attn_batch8.hip.
// yume_attn_fwd_band (sliding-window / causal attention) has the banded form of attn_fwd_kernel_v2: attn_band.hpp, planned by attn_band_plan.hpp.
// yume_attn_fwd_fband (frame-window / frame-causal attention over a block partition) has that walk with another interval source: attn_fband.hpp,
// planned by attn_fband_plan.hpp. yume_attn_fwd_fsink adds an always-visible sink of leading blocks: a walk over a tile LIST, attn_fsink.hpp,
// planned by attn_fsink_plan.hpp. yume_attn_fwd_fprefix is the frame window over two key buffers, an always-visible prefix in a buffer of
// its own and the suffix under the window: attn_fprefix.hpp, planned by attn_fprefix_plan.hpp.
// and attn_combine_kernel (attn_combine.hpp) merges the key-range pieces of a split v7 / v8 launch, planned by attn_plan.hpp.
// The transposed formulation and the tile layouts the kernels share: attn_tile.hpp.
#include "common.hpp"
#include "attn_args.hpp"
#include "counters.hpp"
#include "attn_plan.hpp"
#include "attn_fwd_v1.hpp"
#include "attn_fwd_v2.hpp"
#include "attn_fwd_v4.hpp"
#include "attn_combine.hpp"
#include "attn_cross_rk.hpp"
#include "attn_short.hpp"
#include "attn_seg.hpp"
#include "attn_band.hpp"
#include "attn_fband.hpp"
#include "attn_fsink.hpp"
#include "attn_fprefix.hpp"
#include <math.h>

static_assert(attn_plan::QBLOCK == QB4 && attn_plan::KTILE == KT && attn_plan::HDIM == D, "attn_plan.hpp restates the tile constants");

// ---- environment switches (read once) ---------------------------------------------------------------------------------------------------
static bool attn8_enabled() {
    static const bool on = [] { const char* v = getenv("YUME_ATTN_V8"); return !v || atoi(v) != 0; }();
    return on;
}
#ifndef YUME_ATTN_SHORT_DEFAULT
// measured (profiles/r7_dedup_pad_keys.md, Lk 78, last key x 435): 32.9 against 53.7 us on the 5B shape, 146.5 against 271.7 us on the 14B
// shape for the 4-wave kernel: faster on both, so variant 0 takes the short-key kernel
#define YUME_ATTN_SHORT_DEFAULT true
#endif
// variant 0 sends a weighted call with Lk <= 128 to the short-key kernel (attn_short.hpp): it measured faster than the 4-wave kernel on both
// cross-attention shapes (the routing rule and the table: profiles/r7_dedup_pad_keys.md). YUME_ATTN_SHORT=0 keeps variant 0 on the 4-wave kernel (A/B runs).
static bool attn_short_auto() {
    static const bool on = [] { const char* v = getenv("YUME_ATTN_SHORT"); return v ? atoi(v) != 0 : YUME_ATTN_SHORT_DEFAULT; }();
    return on;
}
// YUME_ATTN_LOG=1: one line per call on stderr with the kernel that takes it (and, for the planned kernels, the plan): what
// tests/test_attn_routes_gpu.py reads back
static bool attn_log_on() {
    static const bool on = [] { const char* v = getenv("YUME_ATTN_LOG"); return v && atoi(v) != 0; }();
    return on;
}
static int cu_count() {
    static thread_local int n[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!n[dev]) {
        int v = 0;
        n[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return n[dev];
}

// (the call does not know which flags the launches will carry: the larger of the two kernels' needs)
extern "C" int64_t yume_attn_workspace_bytes(int64_t Lq, int64_t Lk, int64_t H) {
    if (Lq <= 0 || Lk <= 0 || H <= 0) return 0;
    auto need = [&](attn_plan::Model m) {
        return attn_plan::applies(m, Lq, Lk) ? attn_plan::workspace_bytes(attn_plan::plan(m, Lq, Lk, H), Lq, H) : 0;
    };
    const int64_t a = need(attn_plan::V7), b = need(attn_plan::V8);
    return a > b ? a : b;
}

// ---- choose: which kernel runs, with which plan ----------------------------------------------------------------------------------------------
enum class Kernel { V1, V2, V2_WEIGHTED, V4, V7, V8, RK, SHORT };
struct Choice {
    Kernel kernel;
    attn_plan::Plan plan;   // V7 / V8: the split the launch carries (splits == 1: whole query blocks only)
    int* counters;          // V8: the counter set of its tickets
};

// the model's plan for the shape where the caller gave the scratch for its partial results, whole query blocks where not
static attn_plan::Plan usable_plan(attn_plan::Model m, const AttnArgs& c, const void* workspace, int64_t workspace_bytes) {
    const attn_plan::Plan pl = attn_plan::plan(m, c.Lq, c.Lk, c.H);
    if (pl.splits > 1 && workspace && workspace_bytes >= attn_plan::workspace_bytes(pl, c.Lq, c.H)) return pl;
    return attn_plan::Plan{(c.Lq + QB4 - 1) / QB4, 1};
}

// Depends on the shape, the flags, the variant, the weight, the scratch, the three environment switches (YUME_ATTN_V8, YUME_ATTN_SHORT and,
// inside attn_rk::applies, YUME_ATTN_RK) and on whether a counter set is there: one is drawn (and consumed) only where the persistent kernel is
// the candidate.
static int choose(const AttnArgs& c, int variant, bool kv_pad, const void* workspace, int64_t workspace_bytes, Choice& out) {
    const attn_plan::Plan none{0, 1};
    const bool weighted = c.last_w != 1.0f;
    // a weighted last key (yume_attn_fwd_kw): the short-key kernel for Lk <= 128, the 4-wave LDS-DMA kernel for any Lk; the other kernels do
    // not take a weight. last_key_weight == 1 changes nothing below.
    if (weighted && (variant == 1 || variant == 4 || variant == 7 || variant == 8 || variant == 9)) {
        yume_set_error("attn_fwd_kw: variant %d does not take a last_key_weight != 1 (variants 0, 2 and 10 do)", variant);
        return YUME_EUNSUP;
    }
    if (variant == 10) {
        YUME_REQUIRE(c.Lk <= attn_short::LKMAX, "attn_fwd: variant 10 (short-key kernel) needs Lk <= 128, got Lk=%lld", (long long)c.Lk);
        YUME_REQUIRE(attn_short::fits(c.Lk, c.ldo, c.O), "attn_fwd: variant 10 (short-key kernel) needs ldo %% 8 == 0 and a 16-byte aligned O");
    }
    if (variant == 10 || (weighted && variant == 0 && attn_short_auto() && attn_short::fits(c.Lk, c.ldo, c.O))) {
        out = Choice{Kernel::SHORT, none, nullptr};
        return YUME_OK;
    }
    if (weighted) {            // variant 0 / 2, any Lk (also Lk >= 1536): attn_fwd_kernel_v2<true> over all query rows
        out = Choice{Kernel::V2_WEIGHTED, none, nullptr};
        return YUME_OK;
    }
    // the persistent kernel (attn_fwd8.hip): base-free body only, K / V^T padded to whole key tiles (the caller's word: YUME_ATTN_KV_PADDED;
    // ldvt can be checked), a registered counter workspace for its tickets. variant 8 insists on it, variant 0 takes it where it applies.
    const int64_t nt8 = (c.Lk + KT - 1) / KT;
    const bool v8_fits = c.q_prescaled && kv_pad && attn_plan::applies(attn_plan::V8, c.Lq, c.Lk) && c.ldvt >= nt8 * KT &&
                         (int64_t)c.Lq * c.ldq * 2 + 512 < (1ll << 32);      // (its Q' loads address a query row by a 32-bit byte offset from the head's base)
    if (variant == 8) {
        YUME_REQUIRE(v8_fits, "attn_fwd: variant 8 needs YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED, Lk >= 512, Lq >= 256 and ldvt >= %lld",
                     (long long)(nt8 * KT));
    }
    // (variant 0: where attn_fwd7 was the choice. Measured, the 512-key cross-attention — 8 tiles per item, an item boundary every 12 us —
    // stays faster on the 4-wave kernel: 0.101 against 0.132 ms in the bench, profiles/r4_bench_ab_v8_on_off.log)
    if (variant == 8 || (variant == 0 && v8_fits && attn_plan::applies(attn_plan::V7, c.Lq, c.Lk) && attn8_enabled())) {
        int* counters = yume_counters::next_set();
        if (variant == 8) YUME_REQUIRE(counters != nullptr, "attn_fwd: variant 8 needs a registered counter workspace (yume_counter_workspace_init)");
        if (counters) {
            out = Choice{Kernel::V8, usable_plan(attn_plan::V8, c, workspace, workspace_bytes), counters};
            return YUME_OK;
        }
    }
    if (variant == 9) YUME_REQUIRE(attn_rk::fits(c.Lq, c.Lk, c.ldvt, kv_pad), "attn_fwd: variant 9 needs 448 < Lk <= 512 (padded), Lq >= 1024, ldvt >= 512");
    if (variant == 9 || (variant == 0 && attn_rk::applies(c.Lq, c.Lk, c.ldvt, kv_pad))) {
        // the 512-key cross-attention: K and V^T resident in registers, persistent workgroups (attn_cross_rk.hpp, r6)
        out = Choice{Kernel::RK, none, nullptr};
        return YUME_OK;
    }
    const attn_plan::Plan whole{(c.Lq + QB4 - 1) / QB4, 1};
    if (variant == 1) out = Choice{Kernel::V1, none, nullptr};
    else if (variant == 2) out = Choice{Kernel::V2, none, nullptr};
    else if (variant == 4) out = Choice{Kernel::V4, none, nullptr};
    else if (variant == 7) out = Choice{Kernel::V7, whole, nullptr};
    else if (!attn_plan::applies(attn_plan::V7, c.Lq, c.Lk))
        out = Choice{Kernel::V2, none, nullptr};   // few key tiles / few queries: the 4-wave kernel's shorter prologue and smaller blocks win (cross-attention)
    else
        // one-wave-per-SIMD kernel, one 256-query workgroup per CU; the blocks of a partial last round are cut into key ranges
        // when the caller gave the scratch for their partial results
        out = Choice{Kernel::V7, usable_plan(attn_plan::V7, c, workspace, workspace_bytes), nullptr};
    return YUME_OK;
}

// ---- launch --------------------------------------------------------------------------------------------------------------------------------
// the v7 / v8 kernels over all query rows: whole blocks below pl.tail_qb, the rest cut into pl.splits key ranges whose partial results go
// to `workspace` (checked by usable_plan) and through the merge pass
// workgroups of the persistent kernel: one per item (whole block or piece), at most one per CU. b: nqb / tail_qb / splits set
static int v8_workgroups(const AttnArgs& b) {
    int64_t items = 0;
    for (int y = 0; y < 8; ++y) items += (int64_t)((b.H + 7 - y) >> 3) * (b.tail_qb + (int64_t)(b.nqb - b.tail_qb) * b.splits);
    return (int)(items < cu_count() ? items : cu_count());
}

// the YUME_ATTN_LOG line of one yume_attn_fwd / _ws / _kw call
static void log_choice(const Choice& ch, const AttnArgs& a, bool kv_pad, const void* workspace) {
    static const char* const names[] = {"v1", "v2", "v2w", "v4", "v7", "v8", "rk", "short"};
    char plan[96] = "";
    if (ch.kernel == Kernel::V7 || ch.kernel == Kernel::V8) {
        int n = snprintf(plan, sizeof plan, " tail_qb=%lld splits=%d", (long long)ch.plan.tail_qb, ch.plan.splits);
        if (ch.kernel == Kernel::V8) {
            AttnArgs b = whole_blocks(a, QB4);
            if (ch.plan.splits > 1) { b.tail_qb = (int)ch.plan.tail_qb; b.splits = ch.plan.splits; }
            snprintf(plan + n, sizeof plan - n, " nwg=%d", v8_workgroups(b));
        }
    }
    fprintf(stderr, "[attn_fwd] %s%s Lq=%d Lk=%d H=%d ldq=%lld ldk=%lld ldvt=%lld ldo=%lld prescaled=%d kv_padded=%d accumulate=%d last_w=%g ws=%d\n",
            names[(int)ch.kernel], plan, a.Lq, a.Lk, a.H, (long long)a.ldq, (long long)a.ldk, (long long)a.ldvt, (long long)a.ldo, a.q_prescaled,
            kv_pad ? 1 : 0, a.accumulate, (double)a.last_w, workspace ? 1 : 0);
}

static void launch_planned(const Choice& ch, const AttnArgs& a, void* workspace, hipStream_t st) {
    AttnArgs b = whole_blocks(a, QB4);
    const attn_plan::Plan& pl = ch.plan;
    if (pl.splits > 1) {
        b.tail_qb = (int)pl.tail_qb;
        b.splits = pl.splits;
        b.part_o = reinterpret_cast<float*>(workspace);
        b.part_ml = b.part_o + (int64_t)pl.splits * attn_plan::split_rows(pl, a.Lq) * a.H * D;
    }
    if (ch.kernel == Kernel::V8) {
        yume_attn8_launch(b, ch.counters, v8_workgroups(b), st);
    } else {
        yume_attn7_launch(b, st);
    }
    if (b.splits > 1) attn_combine::launch(b, QB4, st);
}

static int attn_fwd_impl(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo, int64_t Lq,
                         int64_t Lk, int64_t H, float scale, int accumulate, int variant, void* workspace, int64_t workspace_bytes,
                         float last_key_weight, void* stream) {
    YUME_REQUIRE(Q && K && Vt && O, "attn_fwd: NULL pointer");
    YUME_REQUIRE(Lq > 0 && Lk > 0 && H > 0, "attn_fwd: empty problem Lq=%lld Lk=%lld H=%lld", (long long)Lq, (long long)Lk, (long long)H);
    YUME_REQUIRE(Lq < (1ll << 30) && Lk < (1ll << 30) && H < 65536, "attn_fwd: dimension too large");
    YUME_REQUIRE((ldq % 8) == 0 && (ldk % 8) == 0 && (ldvt % 8) == 0 && (ldo % 4) == 0, "attn_fwd: ldq/ldk/ldvt must be multiples of 8, ldo of 4");
    YUME_REQUIRE(ldk < (1ll << 24) && ldvt < (1ll << 24), "attn_fwd: ldk / ldvt too large for 32-bit tile offsets");
    YUME_REQUIRE(ldvt >= Lk && ldvt >= 8, "attn_fwd: ldvt=%lld must be >= Lk=%lld", (long long)ldvt, (long long)Lk);
    YUME_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)K % 16) == 0 && ((uintptr_t)Vt % 16) == 0 && ((uintptr_t)O % 8) == 0, "attn_fwd: pointer alignment");
    AttnArgs a{};               // (q_lo 0, no split: nqb / tail_qb / part_o / part_ml are the launch's to set)
    a.Q = (const unsigned short*)Q; a.ldq = ldq;
    a.K = (const unsigned short*)K; a.ldk = ldk;
    a.Vt = (const unsigned short*)Vt; a.ldvt = ldvt;
    a.O = (unsigned short*)O; a.ldo = ldo;
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H;
    // YUME_ATTN_Q_PRESCALED: Q already carries scale * log2(e) (the caller folded it into the producer of Q before its bf16 rounding): the
    // scores are the exponents. `scale` is ignored; every kernel sees scale_log2 = 1, the one-wave-per-SIMD kernel runs its base-free pieces.
    const int q_pre = (variant & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (variant & YUME_ATTN_KV_PADDED) != 0;
    variant &= ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    a.q_prescaled = q_pre;
    a.scale_log2 = q_pre ? 1.0f : scale * 1.4426950408889634f;
    a.accumulate = accumulate;
    a.splits = 1;
    a.last_w = last_key_weight;
    hipStream_t st = (hipStream_t)stream;

    Choice ch;
    const int rc = choose(a, variant, kv_pad != 0, workspace, workspace_bytes, ch);
    if (rc != YUME_OK) return rc;
    if (attn_log_on()) log_choice(ch, a, kv_pad != 0, workspace);

    switch (ch.kernel) {
        case Kernel::SHORT: attn_short::launch(a, cu_count(), st); break;
        case Kernel::RK: attn_rk::launch(a, cu_count(), st); break;
        case Kernel::V1: attn_v1::launch(a, st); break;
        case Kernel::V2: attn_v2::launch(a, false, st); break;
        case Kernel::V2_WEIGHTED: attn_v2::launch(a, true, st); break;
        case Kernel::V4: attn_v4::launch(a, st); break;
        case Kernel::V7:
        case Kernel::V8: launch_planned(ch, a, workspace, st); break;
    }
    YUME_CHECK_LAUNCH("attn_fwd");
    return YUME_OK;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int yume_attn_fwd(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                             void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate,
                             int variant, void* stream) {
    return attn_fwd_impl(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, nullptr, 0, 1.0f, stream);
}

extern "C" int yume_attn_fwd_ws(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                                void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate,
                                int variant, void* workspace, int64_t workspace_bytes, void* stream) {
    return attn_fwd_impl(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, workspace, workspace_bytes, 1.0f, stream);
}

extern "C" int yume_attn_fwd_kw(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt,
                                void* O, int64_t ldo, int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate,
                                int variant, void* workspace, int64_t workspace_bytes, float last_key_weight, void* stream) {
    YUME_REQUIRE(isfinite(last_key_weight) && last_key_weight >= 1.0f && last_key_weight <= 1048576.0f,
                 "attn_fwd_kw: last_key_weight=%g must be finite and in [1, 2^20]", (double)last_key_weight);
    return attn_fwd_impl(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, workspace, workspace_bytes, last_key_weight, stream);
}

// Sliding-window / causal attention (attn_band.hpp): row i sits at q_pos0 + i on the key axis and sees the keys of attn_band_plan::visible.
// A window that hides no (row, key) pair of the call IS yume_attn_fwd_ws: same entry, same kernel choice, same bits.
extern "C" int yume_attn_fwd_band(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                                  int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant, int64_t q_pos0, int64_t win_left,
                                  int64_t win_right, void* workspace, int64_t workspace_bytes, void* stream) {
    YUME_REQUIRE(Q && K && Vt && O, "attn_fwd_band: NULL pointer");
    YUME_REQUIRE(Lq > 0 && Lk > 0 && H > 0, "attn_fwd_band: empty problem Lq=%lld Lk=%lld H=%lld", (long long)Lq, (long long)Lk, (long long)H);
    YUME_REQUIRE(Lq < (1ll << 30) && Lk < (1ll << 30) && H < 65536, "attn_fwd_band: dimension too large");
    YUME_REQUIRE((ldq % 8) == 0 && (ldk % 8) == 0 && (ldvt % 8) == 0 && (ldo % 4) == 0, "attn_fwd_band: ldq/ldk/ldvt must be multiples of 8, ldo of 4");
    YUME_REQUIRE(ldk < (1ll << 24) && ldvt < (1ll << 24), "attn_fwd_band: ldk / ldvt too large for 32-bit tile offsets");
    YUME_REQUIRE(ldvt >= Lk && ldvt >= 8, "attn_fwd_band: ldvt=%lld must be >= Lk=%lld", (long long)ldvt, (long long)Lk);
    YUME_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)K % 16) == 0 && ((uintptr_t)Vt % 16) == 0 && ((uintptr_t)O % 8) == 0,
                 "attn_fwd_band: pointer alignment");
    YUME_REQUIRE(win_left >= -1 && win_right >= -1, "attn_fwd_band: win_left=%lld / win_right=%lld must be >= -1 (-1: unbounded on that side)",
                 (long long)win_left, (long long)win_right);
    YUME_REQUIRE(q_pos0 >= -(1ll << 31) && q_pos0 < (1ll << 31), "attn_fwd_band: q_pos0=%lld must be in [-2^31, 2^31)", (long long)q_pos0);
    const attn_band_plan::Window w{q_pos0, win_left, win_right};
    if (attn_band_plan::hides_nothing(Lq, Lk, w))
        return yume_attn_fwd_ws(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, workspace, workspace_bytes, stream);
    const int q_pre = (variant & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (variant & YUME_ATTN_KV_PADDED) != 0;
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 11) {
        yume_set_error("attn_fwd_band: variant %d has no banded kernel (variants 0 and 11 do)", v);
        return YUME_EUNSUP;
    }
    AttnArgs a{};
    a.Q = (const unsigned short*)Q; a.ldq = ldq;
    a.K = (const unsigned short*)K; a.ldk = ldk;
    a.Vt = (const unsigned short*)Vt; a.ldvt = ldvt;
    a.O = (unsigned short*)O; a.ldo = ldo;
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H;
    a.q_prescaled = q_pre;
    a.scale_log2 = q_pre ? 1.0f : scale * 1.4426950408889634f;
    a.accumulate = accumulate;
    a.splits = 1;
    a.last_w = 1.0f;
    if (attn_log_on()) {
        int64_t tmin = INT64_MAX, tmax = 0;
        for (int64_t q = 0; q < Lq; q += QB) {
            const attn_band_plan::TileRange r = attn_band_plan::tile_range(q, (q + QB < Lq ? q + QB : Lq) - 1, Lk, w);
            const int64_t n = r.hi - r.lo + 1;
            tmin = n < tmin ? n : tmin;
            tmax = n > tmax ? n : tmax;
        }
        fprintf(stderr, "[attn_fwd_band] band q_pos0=%lld left=%lld right=%lld tiles_min=%lld tiles_max=%lld Lq=%d Lk=%d H=%d ldq=%lld ldk=%lld "
                        "ldvt=%lld ldo=%lld prescaled=%d kv_padded=%d accumulate=%d\n", (long long)q_pos0, (long long)win_left, (long long)win_right,
                (long long)tmin, (long long)tmax, a.Lq, a.Lk, a.H, (long long)ldq, (long long)ldk, (long long)ldvt, (long long)ldo, q_pre, kv_pad, accumulate);
    }
    attn_band::launch(a, w, (hipStream_t)stream);
    YUME_CHECK_LAUNCH("attn_fwd_band");
    return YUME_OK;
}

// the argument checks of yume_attn_fwd_fband and yume_attn_fwd_fsink, answered under the caller's name; fills the plan, N and NB
static int fband_check(const char* who, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                       int64_t Lq, int64_t Lk, int64_t H, int64_t q_pos0, int64_t nspan, const int64_t* span_rows, const int64_t* span_blocks,
                       int64_t back, int64_t ahead, attn_fband_plan::Plan& w, int64_t& N, int64_t& NB) {
    YUME_REQUIRE(Q && K && Vt && O && span_rows && span_blocks, "%s: NULL pointer", who);
    YUME_REQUIRE(Lq > 0 && Lk > 0 && H > 0, "%s: empty problem Lq=%lld Lk=%lld H=%lld", who, (long long)Lq, (long long)Lk, (long long)H);
    YUME_REQUIRE(Lq < (1ll << 30) && Lk < (1ll << 30) && H < 65536, "%s: dimension too large", who);
    YUME_REQUIRE((ldq % 8) == 0 && (ldk % 8) == 0 && (ldvt % 8) == 0 && (ldo % 4) == 0, "%s: ldq/ldk/ldvt must be multiples of 8, ldo of 4", who);
    YUME_REQUIRE(ldk < (1ll << 24) && ldvt < (1ll << 24), "%s: ldk / ldvt too large for 32-bit tile offsets", who);
    YUME_REQUIRE(ldvt >= Lk && ldvt >= 8, "%s: ldvt=%lld must be >= Lk=%lld", who, (long long)ldvt, (long long)Lk);
    YUME_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)K % 16) == 0 && ((uintptr_t)Vt % 16) == 0 && ((uintptr_t)O % 8) == 0,
                 "%s: pointer alignment", who);
    YUME_REQUIRE(nspan >= 1 && nspan <= attn_fband_plan::MAX_SPANS, "%s: nspan=%lld must be in [1, %d]", who, (long long)nspan,
                 attn_fband_plan::MAX_SPANS);
    w = attn_fband_plan::Plan{};
    w.q_pos0 = q_pos0; w.back = back; w.ahead = ahead; w.nspan = (int32_t)nspan;
    N = 0; NB = 0;
    for (int g = 0; g < (int)nspan; ++g) {
        YUME_REQUIRE(span_rows[g] >= 1 && span_blocks[g] >= 1, "%s: span %d: span_rows=%lld and span_blocks=%lld must be >= 1", who, g,
                     (long long)span_rows[g], (long long)span_blocks[g]);
        YUME_REQUIRE(span_rows[g] < (1ll << 31) && span_blocks[g] < (1ll << 31) && N + span_rows[g] * span_blocks[g] < (1ll << 31),
                     "%s: the partition's N must be below 2^31 rows (span %d)", who, g);
        N += span_rows[g] * span_blocks[g];
        NB += span_blocks[g];
        w.rows[g] = (int32_t)span_rows[g];
        w.nblk[g] = (int32_t)span_blocks[g];
    }
    YUME_REQUIRE(back >= -1 && ahead >= -1, "%s: back=%lld / ahead=%lld must be >= -1 (-1: unbounded on that side)", who, (long long)back,
                 (long long)ahead);
    YUME_REQUIRE(q_pos0 >= 0, "%s: q_pos0=%lld must be >= 0", who, (long long)q_pos0);
    YUME_REQUIRE(q_pos0 + Lq <= N, "%s: q_pos0=%lld + Lq=%lld rows end behind the partition's N=%lld", who, (long long)q_pos0, (long long)Lq,
                 (long long)N);
    YUME_REQUIRE(Lk <= N, "%s: Lk=%lld keys exceed the partition's N=%lld", who, (long long)Lk, (long long)N);
    return YUME_OK;
}

static AttnArgs band_args(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo, int64_t Lq,
                          int64_t Lk, int64_t H, float scale, int accumulate, int q_pre) {
    AttnArgs a{};
    a.Q = (const unsigned short*)Q; a.ldq = ldq;
    a.K = (const unsigned short*)K; a.ldk = ldk;
    a.Vt = (const unsigned short*)Vt; a.ldvt = ldvt;
    a.O = (unsigned short*)O; a.ldo = ldo;
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H;
    a.q_prescaled = q_pre;
    a.scale_log2 = q_pre ? 1.0f : scale * 1.4426950408889634f;
    a.accumulate = accumulate;
    a.splits = 1;
    a.last_w = 1.0f;
    return a;
}

// Frame-window / frame-causal attention (attn_fband.hpp): the key axis is partitioned into blocks by nspan uniform spans (host arrays, copied
// into the kernel arguments); row i sits at q_pos0 + i and sees every key of the blocks within `back` before and `ahead` after its own
// (attn_fband_plan::visible). A (partition, back, ahead, q_pos0) that hides no (row, key) pair of the call IS yume_attn_fwd_ws.
extern "C" int yume_attn_fwd_fband(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                                   int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant, int64_t q_pos0, int64_t nspan,
                                   const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    attn_fband_plan::Plan w;
    int64_t N, NB;
    const int rc = fband_check("attn_fwd_fband", Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, q_pos0, nspan, span_rows, span_blocks, back, ahead, w, N, NB);
    if (rc != YUME_OK) return rc;
    if (attn_fband_plan::hides_nothing(Lq, Lk, w))
        return yume_attn_fwd_ws(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, workspace, workspace_bytes, stream);
    const int q_pre = (variant & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (variant & YUME_ATTN_KV_PADDED) != 0;
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 12) {
        yume_set_error("attn_fwd_fband: variant %d has no frame-banded kernel (variants 0 and 12 do)", v);
        return YUME_EUNSUP;
    }
    const AttnArgs a = band_args(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, q_pre);
    if (attn_log_on()) {
        int64_t tmin = INT64_MAX, tmax = 0;
        for (int64_t q = 0; q < Lq; q += QB) {
            const attn_fband_plan::TileRange r = attn_fband_plan::tile_range(q, (q + QB < Lq ? q + QB : Lq) - 1, Lk, w);
            const int64_t n = r.hi - r.lo + 1;
            tmin = n < tmin ? n : tmin;
            tmax = n > tmax ? n : tmax;
        }
        fprintf(stderr, "[attn_fwd_fband] fband q_pos0=%lld back=%lld ahead=%lld nspan=%lld nblocks=%lld tiles_min=%lld tiles_max=%lld Lq=%d Lk=%d "
                        "H=%d ldq=%lld ldk=%lld ldvt=%lld ldo=%lld prescaled=%d kv_padded=%d accumulate=%d\n", (long long)q_pos0, (long long)back,
                (long long)ahead, (long long)nspan, (long long)NB, (long long)tmin, (long long)tmax, a.Lq, a.Lk, a.H, (long long)ldq, (long long)ldk,
                (long long)ldvt, (long long)ldo, q_pre, kv_pad, accumulate);
    }
    attn_fband::launch(a, w, (hipStream_t)stream);
    YUME_CHECK_LAUNCH("attn_fwd_fband");
    return YUME_OK;
}

// The frame window with an always-visible sink (attn_fsink.hpp): the first `sink` blocks of the partition are seen by every row
// (attn_fsink_plan::visible). A call that hides nothing IS yume_attn_fwd_ws; a sink that shows nothing the window hides IS
// yume_attn_fwd_fband; only a call whose sink adds a pair runs the kernel.
extern "C" int yume_attn_fwd_fsink(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                                   int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant, int64_t q_pos0, int64_t nspan,
                                   const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead, int64_t sink,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    attn_fband_plan::Plan w;
    int64_t N, NB;
    const int rc = fband_check("attn_fwd_fsink", Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, q_pos0, nspan, span_rows, span_blocks, back, ahead, w, N, NB);
    if (rc != YUME_OK) return rc;
    YUME_REQUIRE(sink >= 0 && sink <= NB, "attn_fwd_fsink: sink=%lld must be in [0, NB=%lld] (the leading blocks every row sees)", (long long)sink,
                 (long long)NB);
    if (attn_fsink_plan::hides_nothing(Lq, Lk, w, sink))
        return yume_attn_fwd_ws(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, workspace, workspace_bytes, stream);
    if (sink == 0 || attn_fsink_plan::adds_nothing(Lq, Lk, w, sink))
        return yume_attn_fwd_fband(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, q_pos0, nspan, span_rows, span_blocks,
                                   back, ahead, workspace, workspace_bytes, stream);
    const int q_pre = (variant & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (variant & YUME_ATTN_KV_PADDED) != 0;
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 13) {
        yume_set_error("attn_fwd_fsink: variant %d has no frame-sink kernel (variants 0 and 13 do)", v);
        return YUME_EUNSUP;
    }
    const AttnArgs a = band_args(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, q_pre);
    if (attn_log_on()) {
        int64_t tmin = INT64_MAX, tmax = 0;
        for (int64_t q = 0; q < Lq; q += QB) {
            const int64_t n = attn_fsink_plan::tile_count(attn_fsink_plan::tile_list(q, (q + QB < Lq ? q + QB : Lq) - 1, Lk, w, sink));
            tmin = n < tmin ? n : tmin;
            tmax = n > tmax ? n : tmax;
        }
        fprintf(stderr, "[attn_fwd_fsink] fsink q_pos0=%lld back=%lld ahead=%lld sink=%lld sink_rows=%lld nspan=%lld nblocks=%lld tiles_min=%lld "
                        "tiles_max=%lld Lq=%d Lk=%d H=%d ldq=%lld ldk=%lld ldvt=%lld ldo=%lld prescaled=%d kv_padded=%d accumulate=%d\n",
                (long long)q_pos0, (long long)back, (long long)ahead, (long long)sink, (long long)attn_fsink_plan::send(Lk, w, sink), (long long)nspan,
                (long long)NB, (long long)tmin, (long long)tmax, a.Lq, a.Lk, a.H, (long long)ldq, (long long)ldk, (long long)ldvt, (long long)ldo, q_pre,
                kv_pad, accumulate);
    }
    attn_fsink::launch(a, w, sink, (hipStream_t)stream);
    YUME_CHECK_LAUNCH("attn_fwd_fsink");
    return YUME_OK;
}

// The frame window over two key buffers (attn_fprefix.hpp): every row sees the n_prefix keys of Kp / Vtp, and the keys of K / Vt that
// yume_attn_fwd_fband's rule shows it (K / Vt / Lk / the spans / back / ahead / q_pos0 describe that suffix, numbered from 0). n_prefix == 0 IS
// yume_attn_fwd_fband with the suffix arguments; every n_prefix >= 1 runs the kernel (there is no one-buffer call to forward to).
extern "C" int yume_attn_fwd_fprefix(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                                     int64_t Lq, int64_t Lk, int64_t H, float scale, int accumulate, int variant, int64_t q_pos0, int64_t nspan,
                                     const int64_t* span_rows, const int64_t* span_blocks, int64_t back, int64_t ahead, const void* Kp,
                                     int64_t ldkp, const void* Vtp, int64_t ldvtp, int64_t n_prefix, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    attn_fband_plan::Plan w;
    int64_t N, NB;
    const int rc = fband_check("attn_fwd_fprefix", Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, q_pos0, nspan, span_rows, span_blocks, back, ahead, w, N, NB);
    if (rc != YUME_OK) return rc;
    YUME_REQUIRE(n_prefix >= 0, "attn_fwd_fprefix: n_prefix=%lld must be >= 0", (long long)n_prefix);
    YUME_REQUIRE(n_prefix < (1ll << 31) && n_prefix + N < (1ll << 31), "attn_fwd_fprefix: n_prefix=%lld + the partition's N=%lld must be below 2^31",
                 (long long)n_prefix, (long long)N);
    if (n_prefix == 0)
        return yume_attn_fwd_fband(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, variant, q_pos0, nspan, span_rows, span_blocks,
                                   back, ahead, workspace, workspace_bytes, stream);
    YUME_REQUIRE(Kp && Vtp, "attn_fwd_fprefix: NULL pointer (Kp / Vtp with n_prefix=%lld)", (long long)n_prefix);
    YUME_REQUIRE((ldkp % 8) == 0 && (ldvtp % 8) == 0, "attn_fwd_fprefix: ldkp / ldvtp must be multiples of 8");
    YUME_REQUIRE(ldkp < (1ll << 24) && ldvtp < (1ll << 24), "attn_fwd_fprefix: ldkp / ldvtp too large for 32-bit tile offsets");
    YUME_REQUIRE(ldvtp >= n_prefix && ldvtp >= 8, "attn_fwd_fprefix: ldvtp=%lld must be >= n_prefix=%lld", (long long)ldvtp, (long long)n_prefix);
    YUME_REQUIRE(((uintptr_t)Kp % 16) == 0 && ((uintptr_t)Vtp % 16) == 0, "attn_fwd_fprefix: pointer alignment (Kp / Vtp)");
    const int q_pre = (variant & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (variant & YUME_ATTN_KV_PADDED) != 0;
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 14) {
        yume_set_error("attn_fwd_fprefix: variant %d has no frame-prefix kernel (variants 0 and 14 do)", v);
        return YUME_EUNSUP;
    }
    const AttnArgs a = band_args(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq, Lk, H, scale, accumulate, q_pre);
    if (attn_log_on()) {
        int64_t tmin = INT64_MAX, tmax = 0;
        for (int64_t q = 0; q < Lq; q += QB) {
            const int64_t n = attn_fsink_plan::tile_count(attn_fprefix_plan::tile_list(q, (q + QB < Lq ? q + QB : Lq) - 1, Lk, w, n_prefix));
            tmin = n < tmin ? n : tmin;
            tmax = n > tmax ? n : tmax;
        }
        fprintf(stderr, "[attn_fwd_fprefix] fprefix n_prefix=%lld prefix_tiles=%lld q_pos0=%lld back=%lld ahead=%lld nspan=%lld nblocks=%lld "
                        "tiles_min=%lld tiles_max=%lld Lq=%d Lk=%d H=%d ldq=%lld ldk=%lld ldvt=%lld ldkp=%lld ldvtp=%lld ldo=%lld prescaled=%d "
                        "kv_padded=%d accumulate=%d\n", (long long)n_prefix, (long long)attn_fprefix_plan::prefix_tiles(n_prefix), (long long)q_pos0,
                (long long)back, (long long)ahead, (long long)nspan, (long long)NB, (long long)tmin, (long long)tmax, a.Lq, a.Lk, a.H, (long long)ldq,
                (long long)ldk, (long long)ldvt, (long long)ldkp, (long long)ldvtp, (long long)ldo, q_pre, kv_pad, accumulate);
    }
    attn_fprefix::launch(a, w, Kp, ldkp, Vtp, ldvtp, n_prefix, (hipStream_t)stream);
    YUME_CHECK_LAUNCH("attn_fwd_fprefix");
    return YUME_OK;
}

// Segmented cross-attention (attn_seg.hpp): nseg independent problems of Lq_seg queries each, seg_pitch rows apart in Q and O, every one with
// its own K / V^T / Lk / last-key weight (host arrays, copied into the kernel arguments). nseg == 1 IS yume_attn_fwd_kw.
extern "C" int yume_attn_fwd_seg(const void* Q, int64_t ldq, const void* const* K, int64_t ldk, const void* const* Vt, int64_t ldvt,
                                 void* O, int64_t ldo, int64_t nseg, int64_t Lq_seg, int64_t seg_pitch, const int64_t* Lk, int64_t H,
                                 float scale, int accumulate, int variant, const float* last_key_weight, void* stream) {
    YUME_REQUIRE(nseg >= 1 && nseg <= ATTN_SEG_MAX, "attn_fwd_seg: nseg=%lld must be in [1, %d]", (long long)nseg, ATTN_SEG_MAX);
    YUME_REQUIRE(Q && K && Vt && O && Lk, "attn_fwd_seg: NULL pointer");
    YUME_REQUIRE(Lq_seg > 0 && H > 0, "attn_fwd_seg: empty problem Lq_seg=%lld H=%lld", (long long)Lq_seg, (long long)H);
    YUME_REQUIRE(seg_pitch >= Lq_seg, "attn_fwd_seg: seg_pitch=%lld must be >= Lq_seg=%lld", (long long)seg_pitch, (long long)Lq_seg);
    YUME_REQUIRE(Lq_seg < (1ll << 30) && seg_pitch * nseg < (1ll << 30) && H < 65536, "attn_fwd_seg: dimension too large");
    YUME_REQUIRE((ldq % 8) == 0 && (ldk % 8) == 0 && (ldvt % 8) == 0 && (ldo % 4) == 0, "attn_fwd_seg: ldq/ldk/ldvt must be multiples of 8, ldo of 4");
    YUME_REQUIRE(ldk < (1ll << 24) && ldvt < (1ll << 24) && ldvt >= 8, "attn_fwd_seg: ldk / ldvt out of range for 32-bit tile offsets");
    YUME_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)O % 8) == 0, "attn_fwd_seg: pointer alignment");
    AttnSegArgs a{};
    int64_t lk_max = 0;
    for (int s = 0; s < (int)nseg; ++s) {
        YUME_REQUIRE(K[s] && Vt[s], "attn_fwd_seg: NULL K / Vt pointer of segment %d", s);
        YUME_REQUIRE(((uintptr_t)K[s] % 16) == 0 && ((uintptr_t)Vt[s] % 16) == 0, "attn_fwd_seg: pointer alignment of segment %d", s);
        YUME_REQUIRE(Lk[s] > 0 && Lk[s] < (1ll << 30), "attn_fwd_seg: Lk[%d]=%lld must be in [1, 2^30)", s, (long long)Lk[s]);
        YUME_REQUIRE(ldvt >= Lk[s], "attn_fwd_seg: ldvt=%lld must be >= Lk[%d]=%lld", (long long)ldvt, s, (long long)Lk[s]);
        const float w = last_key_weight ? last_key_weight[s] : 1.0f;
        YUME_REQUIRE(isfinite(w) && w >= 1.0f && w <= 1048576.0f, "attn_fwd_seg: last_key_weight[%d]=%g must be finite and in [1, 2^20]", s, (double)w);
        a.K[s] = (const unsigned short*)K[s];
        a.Vt[s] = (const unsigned short*)Vt[s];
        a.Lk[s] = (int)Lk[s];
        a.last_w[s] = w;
        lk_max = Lk[s] > lk_max ? Lk[s] : lk_max;
    }
    const int flags = variant & (YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 2 && v != 10) {
        yume_set_error("attn_fwd_seg: variant %d has no segmented kernel (variants 0, 2 and 10 do)", v);
        return YUME_EUNSUP;
    }
    if (v == 10) YUME_REQUIRE(lk_max <= attn_short::LKMAX, "attn_fwd_seg: variant 10 (short-key kernel) needs every Lk <= 128, got %lld", (long long)lk_max);
    if (nseg == 1)      // one segment is the plain weighted call: same kernel choice, same bits
        return yume_attn_fwd_kw(Q, ldq, K[0], ldk, Vt[0], ldvt, O, ldo, Lq_seg, Lk[0], H, scale, accumulate, v | flags, nullptr, 0, a.last_w[0], stream);
    a.Q = (const unsigned short*)Q; a.ldq = ldq; a.ldk = ldk; a.ldvt = ldvt;
    a.O = (unsigned short*)O; a.ldo = ldo;
    a.nseg = (int)nseg; a.Lq_seg = (int)Lq_seg; a.seg_pitch = (int)seg_pitch; a.H = (int)H;
    a.scale_log2 = (flags & YUME_ATTN_Q_PRESCALED) ? 1.0f : scale * 1.4426950408889634f;
    a.accumulate = accumulate;
    hipStream_t st = (hipStream_t)stream;
    const bool fits = attn_seg::short_fits(a);
    if (v == 10) YUME_REQUIRE(fits, "attn_fwd_seg: variant 10 (short-key kernel) needs ldo %% 8 == 0 and a 16-byte aligned O");
    const bool seg_short = v == 10 || (v == 0 && fits && attn_short_auto());
    if (attn_log_on()) {
        fprintf(stderr, "[attn_fwd_seg] %s nseg=%d Lq_seg=%d seg_pitch=%d H=%d Lk=", seg_short ? "seg_short" : "seg_v2", a.nseg, a.Lq_seg, a.seg_pitch, a.H);
        for (int s = 0; s < a.nseg; ++s) fprintf(stderr, "%s%d", s ? "," : "", a.Lk[s]);
        fprintf(stderr, " ldq=%lld ldk=%lld ldvt=%lld ldo=%lld prescaled=%d kv_padded=%d accumulate=%d\n", (long long)ldq, (long long)ldk,
                (long long)ldvt, (long long)ldo, (flags & YUME_ATTN_Q_PRESCALED) ? 1 : 0, (flags & YUME_ATTN_KV_PADDED) ? 1 : 0, accumulate);
    }
    if (seg_short) attn_seg::launch_short(a, cu_count(), st);
    else attn_seg::launch_v2(a, st);
    YUME_CHECK_LAUNCH("attn_fwd_seg");
    return YUME_OK;
}

// Batched self-attention (attn_batch8.hip): nseg problems of one shape stacked in the same Q / K / V^T / O buffers, q_pitch rows (Q, O) and
// k_pitch rows (K) / columns (V^T) apart. nseg == 1 IS yume_attn_fwd_ws.
static int64_t ceil_tile(int64_t Lk) { return (Lk + KT - 1) / KT * KT; }

extern "C" int64_t yume_attn_batch_workspace_bytes(int64_t nseg, int64_t Lq_seg, int64_t Lk_seg, int64_t H) {
    if (nseg <= 0 || Lq_seg <= 0 || Lk_seg <= 0 || H <= 0) return 0;
    if (nseg == 1) return yume_attn_workspace_bytes(Lq_seg, Lk_seg, H);
    if (!attn_plan::applies(attn_plan::V8, Lq_seg, Lk_seg)) return 0;
    // one plan for the nseg * H virtual heads; every segment has its own slice of partial results
    return nseg * attn_plan::workspace_bytes(attn_plan::plan(attn_plan::V8, Lq_seg, Lk_seg, nseg * H), Lq_seg, H);
}

extern "C" int yume_attn_fwd_batch(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* Vt, int64_t ldvt, void* O, int64_t ldo,
                                   int64_t nseg, int64_t Lq_seg, int64_t q_pitch, int64_t Lk_seg, int64_t k_pitch, int64_t H, float scale,
                                   int accumulate, int variant, void* workspace, int64_t workspace_bytes, void* stream) {
    YUME_REQUIRE(nseg >= 1 && nseg <= ATTN_SEG_MAX, "attn_fwd_batch: nseg=%lld must be in [1, %d]", (long long)nseg, ATTN_SEG_MAX);
    YUME_REQUIRE(Q && K && Vt && O, "attn_fwd_batch: NULL pointer");
    YUME_REQUIRE(Lq_seg > 0 && Lk_seg > 0 && H > 0, "attn_fwd_batch: empty problem Lq_seg=%lld Lk_seg=%lld H=%lld", (long long)Lq_seg,
                 (long long)Lk_seg, (long long)H);
    YUME_REQUIRE(Lq_seg < (1ll << 30) && Lk_seg < (1ll << 30) && H < 65536 / ATTN_SEG_MAX, "attn_fwd_batch: dimension too large");
    YUME_REQUIRE(q_pitch >= Lq_seg && q_pitch * nseg < (1ll << 30), "attn_fwd_batch: q_pitch=%lld must be >= Lq_seg=%lld (and nseg * q_pitch < 2^30)",
                 (long long)q_pitch, (long long)Lq_seg);
    YUME_REQUIRE((k_pitch % KT) == 0 && k_pitch >= ceil_tile(Lk_seg) && k_pitch * nseg < (1ll << 30),
                 "attn_fwd_batch: k_pitch=%lld must be a multiple of 64 and >= %lld (Lk_seg=%lld in whole key tiles)", (long long)k_pitch,
                 (long long)ceil_tile(Lk_seg), (long long)Lk_seg);
    YUME_REQUIRE((ldq % 8) == 0 && (ldk % 8) == 0 && (ldvt % 8) == 0 && (ldo % 4) == 0, "attn_fwd_batch: ldq/ldk/ldvt must be multiples of 8, ldo of 4");
    YUME_REQUIRE(ldk < (1ll << 24) && ldvt < (1ll << 24), "attn_fwd_batch: ldk / ldvt too large for 32-bit tile offsets");
    YUME_REQUIRE(ldvt >= (nseg - 1) * k_pitch + ceil_tile(Lk_seg), "attn_fwd_batch: ldvt=%lld must be >= (nseg-1)*k_pitch + Lk_seg in whole key tiles = %lld",
                 (long long)ldvt, (long long)((nseg - 1) * k_pitch + ceil_tile(Lk_seg)));
    YUME_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)K % 16) == 0 && ((uintptr_t)Vt % 16) == 0 && ((uintptr_t)O % 16) == 0,
                 "attn_fwd_batch: pointer alignment (Q, K, Vt, O: 16 bytes)");
    const int flags = variant & (YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    const int v = variant & ~(YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED);
    if (v != 0 && v != 2 && v != 8) {
        yume_set_error("attn_fwd_batch: variant %d has no batch kernel (variants 0, 2 and 8 do)", v);
        return YUME_EUNSUP;
    }
    const int64_t ws_need = yume_attn_batch_workspace_bytes(nseg, Lq_seg, Lk_seg, H);
    if (workspace) {
        YUME_REQUIRE(((uintptr_t)workspace % 16) == 0, "attn_fwd_batch: workspace must be 16-byte aligned");
        YUME_REQUIRE(workspace_bytes >= ws_need, "attn_fwd_batch: workspace_bytes=%lld is below yume_attn_batch_workspace_bytes = %lld",
                     (long long)workspace_bytes, (long long)ws_need);
    }
    if (nseg == 1)      // one segment is the plain call: same kernel choice, same bits
        return yume_attn_fwd_ws(Q, ldq, K, ldk, Vt, ldvt, O, ldo, Lq_seg, Lk_seg, H, scale, accumulate, variant, workspace, workspace_bytes, stream);

    const bool q_pre = (flags & YUME_ATTN_Q_PRESCALED) != 0, kv_pad = (flags & YUME_ATTN_KV_PADDED) != 0;
    hipStream_t st = (hipStream_t)stream;
    // the persistent kernel's own conditions, for ONE segment's extent (the segments' bases are 64-bit)
    const bool p8_fits = q_pre && kv_pad && attn_plan::applies(attn_plan::V8, Lq_seg, Lk_seg) && Lq_seg * ldq * 2 + 512 < (1ll << 32);
    if (v == 8)
        YUME_REQUIRE(p8_fits, "attn_fwd_batch: variant 8 needs YUME_ATTN_Q_PRESCALED | YUME_ATTN_KV_PADDED, Lk_seg >= 512, Lq_seg >= 256 and "
                              "Lq_seg * ldq < 2^31");
    int* counters = nullptr;
    if (v == 8 || (v == 0 && p8_fits && attn_plan::applies(attn_plan::V7, Lq_seg, Lk_seg) && attn8_enabled())) {
        counters = yume_counters::next_set();
        if (v == 8) YUME_REQUIRE(counters != nullptr, "attn_fwd_batch: variant 8 needs a registered counter workspace (yume_counter_workspace_init)");
    }
    if (counters) {
        AttnArgs a{};
        a.Q = (const unsigned short*)Q; a.ldq = ldq;
        a.K = (const unsigned short*)K; a.ldk = ldk;
        a.Vt = (const unsigned short*)Vt; a.ldvt = ldvt;
        a.O = (unsigned short*)O; a.ldo = ldo;
        a.Lq = (int)Lq_seg; a.Lk = (int)Lk_seg; a.H = (int)(nseg * H);        // virtual heads: what the queues and the plan see
        a.q_prescaled = 1;
        a.scale_log2 = 1.0f;
        a.accumulate = accumulate;
        a.splits = 1;
        a.last_w = 1.0f;
        AttnArgs b = whole_blocks(a, QB4);
        attn_plan::Plan pl = attn_plan::plan(attn_plan::V8, Lq_seg, Lk_seg, nseg * H);
        if (pl.splits > 1 && !workspace) pl = attn_plan::Plan{(Lq_seg + QB4 - 1) / QB4, 1};      // no scratch: whole query blocks
        AttnBatchSeg sg{};
        sg.H = (int)H;
        sg.q_step = q_pitch * ldq; sg.k_step = k_pitch * ldk; sg.o_step = q_pitch * ldo; sg.vt_step = k_pitch;
        if (pl.splits > 1) {
            const int64_t rows = attn_plan::split_rows(pl, Lq_seg);
            b.tail_qb = (int)pl.tail_qb;
            b.splits = pl.splits;
            sg.part_o_step = (int64_t)pl.splits * rows * H * D;
            sg.part_ml_step = (int64_t)pl.splits * rows * H * 2;
            b.part_o = reinterpret_cast<float*>(workspace);
            b.part_ml = b.part_o + nseg * sg.part_o_step;
        }
        const int nwg = v8_workgroups(b);
        if (attn_log_on())
            fprintf(stderr, "[attn_fwd_batch] batch_v8 tail_qb=%lld splits=%d nwg=%d nseg=%d Lq_seg=%d q_pitch=%lld Lk_seg=%d k_pitch=%lld H=%d ldq=%lld "
                            "ldk=%lld ldvt=%lld ldo=%lld accumulate=%d ws=%d\n", (long long)pl.tail_qb, pl.splits, nwg, (int)nseg, a.Lq, (long long)q_pitch,
                    a.Lk, (long long)k_pitch, (int)H, (long long)ldq, (long long)ldk, (long long)ldvt, (long long)ldo, accumulate, workspace ? 1 : 0);
        yume_attn_batch8_launch(b, sg, counters, nwg, st);
        if (b.splits > 1) {
            // the merge pass as it stands, once per segment: that segment's slice of the partial results, its O rows, H heads
            for (int s = 0; s < (int)nseg; ++s) {
                AttnArgs c = b;
                c.H = (int)H;
                c.O = b.O + s * sg.o_step;
                c.part_o = b.part_o + s * sg.part_o_step;
                c.part_ml = b.part_ml + s * sg.part_ml_step;
                attn_combine::launch(c, QB4, st);
            }
        }
        YUME_CHECK_LAUNCH("attn_fwd_batch");
        return YUME_OK;
    }
    // the 4-wave segmented kernel (attn_seg.hpp) with K[s] / Vt[s] pointing into the stacked buffers and weights of 1
    AttnSegArgs g{};
    g.Q = (const unsigned short*)Q; g.ldq = ldq; g.ldk = ldk; g.ldvt = ldvt;
    g.O = (unsigned short*)O; g.ldo = ldo;
    for (int s = 0; s < (int)nseg; ++s) {
        g.K[s] = (const unsigned short*)K + s * k_pitch * ldk;
        g.Vt[s] = (const unsigned short*)Vt + s * k_pitch;
        g.Lk[s] = (int)Lk_seg;
        g.last_w[s] = 1.0f;
    }
    g.nseg = (int)nseg; g.Lq_seg = (int)Lq_seg; g.seg_pitch = (int)q_pitch; g.H = (int)H;
    g.scale_log2 = q_pre ? 1.0f : scale * 1.4426950408889634f;
    g.accumulate = accumulate;
    if (attn_log_on())
        fprintf(stderr, "[attn_fwd_batch] seg_v2 nseg=%d Lq_seg=%d q_pitch=%lld Lk_seg=%d k_pitch=%lld H=%d ldq=%lld ldk=%lld ldvt=%lld ldo=%lld "
                        "prescaled=%d kv_padded=%d accumulate=%d\n", (int)nseg, (int)Lq_seg, (long long)q_pitch, (int)Lk_seg, (long long)k_pitch, (int)H,
                (long long)ldq, (long long)ldk, (long long)ldvt, (long long)ldo, q_pre ? 1 : 0, kv_pad ? 1 : 0, accumulate);
    attn_seg::launch_v2(g, st);
    YUME_CHECK_LAUNCH("attn_fwd_batch");
    return YUME_OK;
}
