// Host-side plan of a grouped weight-gradient launch, shared by size query, launch and plan query (LABNOTES R19.1).  No HIP types.
#pragma once
#include <stdint.h>
#include "../../include/sais_hip.h"

constexpr int TK = 64, WQ = 384;                 // 128-row tiles: m rows per step; wide form: 128 x 384 tiles, from M = TN_MIN_M on
constexpr int XP = 192, XQ = 384, XK = 32, XL_MIN_STEPS = 48;   // XL form: 192 x 384 tiles, 32-row steps, >= 48 of them per M-split
constexpr int TN_MIN_M = 8192, TN_ONE_ROUND = 256;   // fewer rows: 128 x 128 tiles; XL and wide: one workgroup per CU, one round
constexpr int F32_OWNER64_MAX_TILES = 200;       // fp32, one M-split, fewer 128-row tiles (the temporal layers: 132): 64-row tiles

enum TnForm { TN_XL_SLAB, TN_XL_ATOMIC, TN_WIDE_SLAB, TN_WIDE_ATOMIC, TN_TILE128, TN_F32_OWNER64, TN_F32_OWNER128, TN_F32_ATOMIC };
struct TnSwitches { int xl_waves; bool xl_slabs, old_slabs; };   // SAIS_TN_XL (0 under SAIS_TN_SLABS), SAIS_TN_XL_SLABS, SAIS_TN_SLABS
struct TnPlan {
    int form, tiles, nsplit, rows, workgroups;   // rows per M-split (XL shares 32-row steps out evenly: the smaller share)
    size_t slab_bytes;                           // what the form uses of the offer (0: no slabs)
    bool short_offer;                            // a slab form applies, the offer is too small for it: its atomic form is planned
};
constexpr int64_t TN_NO_SLABS = -1, TN_ANY_SLABS = INT64_MAX;      // offers: no slab buffer / whatever the form needs (size query)
// XL slabs per workgroup: the raw fp32 tile + one 32 x 32 bias tile per wave; gemm_tn_xl.hip checks a plan against its own wave count
constexpr size_t xl_slab_bytes_per_wg(int nwaves) { return (size_t)XP * XQ * 4 + (size_t)nwaves * 32 * 32 * 4; }
// gemm_tn_xl.hip: the launch of the XL form of `pl`; slabs = NULL: fp32 atomics.  gemm_tn.hip: the plan for an offer, without a launch
int sais_tn_xl_launch(const TnPlan& pl, const SaisTnItem* items, int nitems, int M, int nwaves, float* slabs, void* stream);
extern "C" int sais_gemm_tn_plan_(const SaisTnItem* items, int nitems, int M, int nsplit, int64_t slab_bytes_offered, int f32, int64_t out[6]);
// M rows cut into at most nsplit slices of `rows` rows, a whole number of TK-row steps each; ns = slices that hold rows
struct TnSplit { int rows, ns; };
static inline TnSplit tn_split(int M, int nsplit) {
    const int rows = ((M + nsplit - 1) / nsplit + TK - 1) / TK * TK;
    return {rows, (M + rows - 1) / rows};
}

// bf16 operands.  nsplit: the caller's M-splits, for the 128 x 128 form only; offer: slab bytes the caller has, or TN_NO_SLABS
static inline TnPlan tn_plan(const SaisTnItem* items, int nitems, int M, int nsplit, int64_t offer, const TnSwitches& sw) {
    bool xl = sw.xl_waves && M % XK == 0 && M >= TN_MIN_M, wide = M % TK == 0 && M >= TN_MIN_M;
    int xt = 0, wt = 0, t128 = 0;
    for (int i = 0; i < nitems; ++i) {
        const SaisTnItem& t = items[i];
        xl = xl && t.N1 % XP == 0 && t.N2 % XQ == 0 && t.ldp % 8 == 0 && t.ldq % 8 == 0 && !(((uintptr_t)t.P | (uintptr_t)t.Q) & 15);
        wide = wide && t.N1 % 128 == 0 && t.N2 % WQ == 0;
        xt += (t.N1 / XP) * (t.N2 / XQ); wt += (t.N1 / 128) * (t.N2 / WQ); t128 += (t.N1 / 128) * (t.N2 / 128);
    }
    TnPlan pl{};
    auto forms = [&](int slab_form, int atomic_form, size_t need) {       // the slab form if it has one (need > 0) and the offer covers it
        const bool slab = need && offer >= 0 && (uint64_t)offer >= need;
        pl.form = slab ? slab_form : atomic_form; pl.slab_bytes = slab ? need : 0;
        pl.short_offer = need && offer >= 0 && !slab; pl.workgroups = pl.tiles * pl.nsplit;
        return pl;
    };
    const int xns = xl && xt > 0 && TN_ONE_ROUND / xt > 1 ? TN_ONE_ROUND / xt : 1;
    if (xl && xt > 0 && M / XK / xns >= XL_MIN_STEPS) {
        pl.tiles = xt; pl.nsplit = xns; pl.rows = M / XK / xns * XK;
        return forms(TN_XL_SLAB, TN_XL_ATOMIC, sw.xl_slabs && xns >= 2 ? xt * xns * xl_slab_bytes_per_wg(sw.xl_waves == 8 ? 8 : 4) : 0);
    }
    if (wide && wt > 0) {
        const TnSplit ws = tn_split(M, TN_ONE_ROUND / wt < 1 ? 1 : TN_ONE_ROUND / wt);
        pl.tiles = wt; pl.nsplit = ws.ns; pl.rows = ws.rows;
        return forms(TN_WIDE_SLAB, TN_WIDE_ATOMIC, sw.old_slabs && ws.ns > 1 ? (size_t)wt * ws.ns * (128 * WQ * 4 + 128 * 4) : 0);
    }
    const TnSplit sp = tn_split(M, nsplit);
    pl.tiles = t128; pl.nsplit = sp.ns; pl.rows = sp.rows;
    return forms(TN_TILE128, TN_TILE128, 0);
}

// fp32 operands (rounded to bf16 while staging): 128 x 128 tiles; one M-split = every tile has one owner, no atomics
static inline TnPlan tn_plan_f32(const SaisTnItem* items, int nitems, int M, int nsplit) {
    const TnSplit sp = tn_split(M, nsplit);
    int t128 = 0, t64 = 0;
    for (int i = 0; i < nitems; ++i) { t128 += (items[i].N1 / 128) * (items[i].N2 / 128); t64 += (items[i].N1 / 64) * (items[i].N2 / 128); }
    const bool owner64 = sp.ns == 1 && t128 < F32_OWNER64_MAX_TILES;
    const int form = owner64 ? TN_F32_OWNER64 : sp.ns == 1 ? TN_F32_OWNER128 : TN_F32_ATOMIC, tiles = owner64 ? t64 : t128;
    return TnPlan{form, tiles, sp.ns, sp.rows, tiles * sp.ns, 0, false};
}
