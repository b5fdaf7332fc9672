// Workspace layouts of the block-level entry points (blocks.hip): offsets, total, split counts (LABNOTES R19.1).  No HIP types.
#pragma once
#include "../../include/sais_hip.h"

constexpr int D = 384, HID = 1536, QKV = 1152, FF = 2048;
constexpr size_t ALIGN = 256;
static inline size_t ws_up(size_t b) { return (b + ALIGN - 1) / ALIGN * ALIGN; }
static inline size_t ws_take(size_t& off, size_t bytes) { const size_t o = off; off += ws_up(bytes); return o; }     // the next region

// SAIS_OP_VIT_BLOCK_BWD: du, d(mid) bf16, d(attention out), dxn (small-M regime), dqkv, then the slabs of the block's grouped dW launch
struct VitBwdLayout { size_t du, dxb, dao, dxn, dqkv, slabs, slab_bytes, total; };
static inline VitBwdLayout vit_bwd_layout(size_t M, size_t dw_slab_bytes) {
    VitBwdLayout l;
    size_t o = 0;
    l.du = ws_take(o, M * HID * 2); l.dxb = ws_take(o, M * D * 2); l.dao = ws_take(o, M * D * 2); l.dxn = ws_take(o, M * D * 2);
    l.dqkv = ws_take(o, M * QKV * 2); l.slabs = ws_take(o, dw_slab_bytes);
    l.slab_bytes = dw_slab_bytes; l.total = o;
    return l;
}
// SAIS_OP_TEMPORAL_LAYER_FWD: one region at offset 0 for the raw split-K slabs of out_proj, then of linear2 (the larger)
struct TemporalFwdLayout { int ns_out, ns_ff; size_t total; };
static inline TemporalFwdLayout temporal_fwd_layout(size_t M) {
    TemporalFwdLayout l = {sais_tgemm_nsplit((int)M, D, D), sais_tgemm_nsplit((int)M, D, FF), 0};
    l.total = ws_up((size_t)(l.ns_ff > l.ns_out ? l.ns_ff : l.ns_out) * M * D * 4);
    return l;
}
// SAIS_OP_TEMPORAL_LAYER_BWD: dy2, dt2 (dropout2's backward of dy2), dt1, dh, dqkv, then the slabs of dh . W1 [ns1][M][384] and, right
// behind them, of dt1 . Wo [nso][M][384].  nsq: splits of dqkv . Win, whose slabs are the caller's (dx_slabs).
struct TemporalBwdLayout { int ns1, nso, nsq; size_t dy2, dt2, dt1, dh, dqkv, slab1, slabo, total; };
static inline TemporalBwdLayout temporal_bwd_layout(size_t M) {
    TemporalBwdLayout l;
    l.ns1 = sais_tgemm_nsplit((int)M, D, FF); l.nso = sais_tgemm_nsplit((int)M, D, D); l.nsq = sais_tgemm_nsplit((int)M, D, QKV);
    size_t o = 0;
    l.dy2 = ws_take(o, M * D * 4); l.dt2 = ws_take(o, M * D * 4); l.dt1 = ws_take(o, M * D * 4); l.dh = ws_take(o, M * FF * 4);
    l.dqkv = ws_take(o, M * QKV * 4); l.slab1 = ws_take(o, (size_t)(l.ns1 + l.nso) * M * D * 4);
    l.slabo = l.slab1 + (size_t)l.ns1 * M * D * 4; l.total = o;
    return l;
}
// S > SAIS_TEMPORAL_MAX_S_BWD: the workspace of the streaming attention backward sits behind that layout (0 bytes up to it)
static inline size_t temporal_long_attn_bytes(int B, int S) {
    return S > SAIS_TEMPORAL_MAX_S_BWD ? ws_up(sais_temporal_attn_long_bwd_workspace_bytes(B, S)) : 0;
}
