// Stand-alone host check of csrc/tn_plan.hpp and csrc/ws_layout.hpp, meant for a sanitizer build (no GPU, no HIP):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tn_plan_check.cpp -o /tmp/tn_plan_check && /tmp/tn_plan_check
// Walks the plan table of tests/test_abi.py (same rows, same hand-written answers) and every shape of tools/host_cmp.py under the
// five switch settings and four kinds of offer, and checks what must hold of any plan and any layout.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../sais_amd/csrc/tn_plan.hpp"
#include "../sais_amd/csrc/ws_layout.hpp"

// stand-in for the library's split rule (tgemm.hip): the layout invariants hold for any counts
extern "C" int sais_tgemm_nsplit(int M, int N, int K) { return 1 + (M + N + K) % 7; }

typedef std::vector<SaisTnItem> Items;
static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); ++bad; } } while (0)

static Items items_of(std::initializer_list<Items> parts) {
    Items v;
    for (const Items& p : parts) v.insert(v.end(), p.begin(), p.end());
    return v;
}
static SaisTnItem shape(int n1, int n2) { return SaisTnItem{nullptr, n1, nullptr, n2, n1, n2, nullptr, n2, nullptr}; }
static Items times(const Items& a, int n) {
    Items v;
    for (int i = 0; i < n; ++i) v.insert(v.end(), a.begin(), a.end());
    return v;
}
static int default_nsplit(const Items& it, int M) {       // ops._tn_nsplit
    int tiles = 0;
    for (const SaisTnItem& t : it) tiles += (t.N1 / 128) * (t.N2 / 128);
    int ns = (432 + tiles - 1) / tiles, cap = (M + 255) / 256;
    ns = ns < cap ? ns : cap;
    return ns < 1 ? 1 : ns;
}

static void row(const TnSwitches& sw, const Items& it, int M, int64_t offer, int form, int wgs, int ns, size_t slab, bool is_short = false) {
    const TnPlan pl = tn_plan(it.data(), (int)it.size(), M, default_nsplit(it, M), offer, sw);
    if (pl.form != form || pl.workgroups != wgs || pl.nsplit != ns || pl.slab_bytes != slab || pl.short_offer != is_short) {
        printf("%zu items M=%d offer=%lld: form %d wgs %d splits %d slab %zu short %d\n", it.size(), M, (long long)offer, pl.form,
               pl.workgroups, pl.nsplit, pl.slab_bytes, pl.short_offer);
        ++bad;
    }
}

int main() {
    const Items BLOCK = {shape(384, 1536), shape(1536, 384), shape(384, 384), shape(1152, 384)}, KV = {shape(768, 384)};
    const Items TEMPORAL = {shape(384, 2048), shape(2048, 384), shape(384, 384), shape(1152, 384)};
    const TnSwitches dflt = {4, true, false}, no_xl = {0, true, false}, xl8 = {8, true, false}, xl_atomic = {4, false, false},
                     old_slabs = {0, true, true};
    const int64_t ANY = TN_ANY_SLABS, NONE = TN_NO_SLABS;
    row(dflt, BLOCK, 50432, ANY, TN_XL_SLAB, 240, 10, 74711040);
    row(dflt, BLOCK, 8192, ANY, TN_WIDE_ATOMIC, 252, 7, 0);
    row(dflt, BLOCK, 12640, ANY, TN_TILE128, 432, 4, 0);
    row(dflt, KV, 50432, ANY, TN_WIDE_ATOMIC, 252, 42, 0);
    row(dflt, items_of({times(BLOCK, 6), KV}), 12608, ANY, TN_XL_ATOMIC, 148, 1, 0);
    row(dflt, items_of({times(BLOCK, 10), KV}), 50432, ANY, TN_XL_ATOMIC, 244, 1, 0);
    row(dflt, {BLOCK[0], BLOCK[1]}, 100864, ANY, TN_XL_SLAB, 256, 16, 79691776);
    row(dflt, {shape(384, 1536), shape(1536, 512)}, 50432, ANY, TN_TILE128, 504, 6, 0);
    row(dflt, {shape(128, 384)}, 50432, ANY, TN_WIDE_ATOMIC, 197, 197, 0);
    row(dflt, BLOCK, 50432, NONE, TN_XL_ATOMIC, 240, 10, 0);
    row(dflt, BLOCK, 50432, 74711040 - 1, TN_XL_ATOMIC, 240, 10, 0, true);
    row(dflt, BLOCK, 50432, 74711040, TN_XL_SLAB, 240, 10, 74711040);
    row(no_xl, BLOCK, 50432, ANY, TN_WIDE_ATOMIC, 252, 7, 0);
    row(xl_atomic, BLOCK, 50432, ANY, TN_XL_ATOMIC, 240, 10, 0);
    row(old_slabs, BLOCK, 50432, ANY, TN_WIDE_SLAB, 252, 7, 49674240);
    row(old_slabs, BLOCK, 50432, NONE, TN_WIDE_ATOMIC, 252, 7, 0);
    row(old_slabs, BLOCK, 50432, 49674240 - 1, TN_WIDE_ATOMIC, 252, 7, 0, true);
    const struct { Items it; int nsplit, form, wgs, ns; } f32rows[] = {{TEMPORAL, 1, TN_F32_OWNER64, 264, 1},
        {times(TEMPORAL, 2), 1, TN_F32_OWNER128, 264, 1}, {TEMPORAL, 2, TN_F32_ATOMIC, 264, 2}};
    for (const auto& r : f32rows) {
        const TnPlan pl = tn_plan_f32(r.it.data(), (int)r.it.size(), 264, r.nsplit);
        CHECK(pl.form == r.form && pl.workgroups == r.wgs && pl.nsplit == r.ns && pl.slab_bytes == 0);
    }

    // every shape of tools/host_cmp.py: what holds of any plan
    const Items sets[] = {BLOCK, {shape(384, 384), shape(1152, 384)}, {shape(384, 1536), shape(1536, 512)}, KV, items_of({times(BLOCK, 6), KV}),
                          items_of({times(BLOCK, 10), KV}), {BLOCK[0], BLOCK[1]}, {shape(128, 384)}, times({shape(384, 384)}, SAIS_TN_MAX_ITEMS)};
    const int Ms[] = {300, 3152, 8192, 12608, 12640, 50432, 100864};
    const TnSwitches sws[] = {dflt, no_xl, xl8, xl_atomic, old_slabs};
    int plans = 0;
    for (const Items& it : sets)
        for (int M : Ms)
            for (const TnSwitches& sw : sws) {
                const int n = (int)it.size(), ns = default_nsplit(it, M);
                const TnPlan need = tn_plan(it.data(), n, M, ns, ANY, sw);
                CHECK(!need.short_offer && need.workgroups == need.tiles * need.nsplit && need.workgroups > 0);
                CHECK((need.slab_bytes != 0) == (need.form == TN_XL_SLAB || need.form == TN_WIDE_SLAB));
                CHECK((long long)need.rows * need.nsplit >= M - (need.form <= TN_XL_ATOMIC ? XK * need.nsplit : 0));
                if (need.form <= TN_WIDE_ATOMIC) CHECK(need.workgroups <= TN_ONE_ROUND || need.nsplit == 1);      // one round of the chip
                const int64_t offers[] = {NONE, 0, (int64_t)need.slab_bytes - 1, (int64_t)need.slab_bytes};
                for (int64_t offer : offers) {
                    const TnPlan pl = tn_plan(it.data(), n, M, ns, offer, sw);
                    CHECK(pl.slab_bytes == 0 || (offer >= 0 && pl.slab_bytes <= (uint64_t)offer));       // never more than offered
                    CHECK(pl.short_offer == (need.slab_bytes && offer >= 0 && (uint64_t)offer < need.slab_bytes));
                    CHECK(pl.tiles == need.tiles && pl.nsplit == need.nsplit && pl.workgroups == need.workgroups);
                    CHECK(pl.form == need.form || (pl.slab_bytes == 0 && pl.form == need.form + 1));      // the slab form or its atomics
                    ++plans;
                }
                const TnPlan f = tn_plan_f32(it.data(), n, M, ns);
                CHECK(f.workgroups == f.tiles * f.nsplit && f.slab_bytes == 0 && f.form >= TN_F32_OWNER64);
            }

    // layouts: regions in order, 256-B aligned, inside the total
    const int shapes[][2] = {{64, 197}, {256, 197}, {16, 37}, {8, 16}, {204, 16}};
    for (const auto& s : shapes)
        for (const TnSwitches& sw : sws) {
            const size_t M = (size_t)s[0] * s[1];
            const VitBwdLayout v = vit_bwd_layout(M, tn_plan(BLOCK.data(), 4, (int)M, 1, ANY, sw).slab_bytes);
            const size_t vo[] = {v.du, v.dxb, v.dao, v.dxn, v.dqkv, v.slabs, v.total};
            for (int i = 0; i < 6; ++i) CHECK(vo[i] < vo[i + 1] + (i == 5) && vo[i] % ALIGN == 0);
            CHECK(v.slabs + v.slab_bytes <= v.total && v.dxb - v.du >= M * HID * 2 && v.slabs - v.dqkv >= M * QKV * 2);
            const TemporalBwdLayout t = temporal_bwd_layout(M);
            const size_t to[] = {t.dy2, t.dt2, t.dt1, t.dh, t.dqkv, t.slab1, t.slabo, t.total};
            for (int i = 0; i < 7; ++i) CHECK(to[i] < to[i + 1] && to[i] % 16 == 0);
            CHECK(t.slabo + (size_t)t.nso * M * D * 4 <= t.total && t.slabo - t.slab1 == (size_t)t.ns1 * M * D * 4);
            const TemporalFwdLayout f = temporal_fwd_layout(M);
            CHECK(f.total >= (size_t)f.ns_out * M * D * 4 && f.total >= (size_t)f.ns_ff * M * D * 4);
        }
    printf("%d plans walked, %d failures\n", plans, bad);
    return bad ? 1 : 0;
}
