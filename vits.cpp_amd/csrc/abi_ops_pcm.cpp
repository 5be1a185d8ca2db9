// abi_ops_pcm.cpp — operator-level entry points of the PCM kernels: vits_op_resample, vits_op_pitch, vits_op_tempo, vits_op_level, vits_op_limit (host arrays in, host arrays out; staging:
// abi_ops_common.h), vits_op_edges (device arrays, as the engine's delivery calls it) and vits_op_join (host arrays; y goes up and comes back).
#include <cmath>

#include "abi_ops_common.h"

using namespace vits;

namespace {
// the polyphase table as the kernels read it: [K][L]
std::vector<float> taps_kl(const ResamplePlan& p) {
    const std::vector<float> h = resample_taps(p);
    std::vector<float> ht(h.size());
    for (int ph = 0; ph < p.L; ++ph)
        for (int k = 0; k < p.K; ++k) ht[(size_t)k * p.L + ph] = h[(size_t)ph * p.K + k];
    return ht;
}
// the rows of a level / limit call: n[b] samples each, the longest; false: a length or y_stride (where y is given) does not fit
bool level_rows(const char* op, const vits_level_desc* d, const int64_t* lens, bool has_y, std::vector<int32_t>& n, int64_t& longest) {
    const std::string at = std::string(op) + ": ";
    n.resize(d->batch);
    longest = 0;
    for (int b = 0; b < d->batch; ++b) {
        const int64_t len = lens ? lens[b] : d->x_stride;
        if (len < 0 || len > d->x_stride) return refuse(at + "lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(d->x_stride) + "]");
        if (len > ((int64_t)1 << 30)) return refuse(at + "row " + std::to_string(b) + " is too long (" + std::to_string(len) + " samples)");
        n[b] = (int32_t)len;
        longest = std::max(longest, len);
    }
    if (has_y && d->y_stride < longest) return refuse(at + "y_stride = " + std::to_string(d->y_stride) + " is shorter than the longest row (" + std::to_string(longest) + " samples)");
    return true;
}
// the engine's staging of PCM rows: a stride of a multiple of 32 samples with a tile to spare, NaN behind every utterance: a read past one shows in the result
int64_t pcm_stride(int64_t longest) { return (longest + 31) / 32 * 32 + 32; }
LevelCall level_call(const vits_level_desc* d, const LoudnessPlan& plan, const DevMem& dx, int64_t xs, const DevMem& dn, int64_t longest, const DevMem& dscr, const DevMem& dlv) {
    LevelCall c;
    c.x = dx.f();
    c.x_stride = xs;
    c.lens = dn.i();
    c.batch = d->batch;
    c.max_len = longest;
    c.plan = plan;
    c.scratch = dscr.f();
    c.kind = d->kind;
    c.value_db = d->value_db;
    c.ceiling_db = d->ceiling_db;
    c.gain = (float)std::pow(10.0, (double)d->value_db / 20.0);
    c.levels = dlv.f();
    return c;
}
}  // namespace

VITS_API int vits_op_resample(int32_t in_rate, int32_t out_rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, float* y, int64_t y_stride) {
    VITS_TRY
    if (batch <= 0 || !x || !y || x_stride <= 0 || y_stride <= 0) return fail("vits_op_resample: null argument or empty batch");
    ResamplePlan p;
    std::string err;
    if (!resample_plan(in_rate, out_rate, p, err)) return fail("vits_op_resample: " + err);
    std::vector<int32_t> n(batch);
    int64_t longest = 0, longest_b = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t len = lens ? lens[b] : x_stride;
        if (len < 0 || len > x_stride) return fail("vits_op_resample: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]");
        if (len > ((int64_t)1 << 30) || p.out_len(len) > INT32_MAX) return fail("vits_op_resample: row " + std::to_string(b) + " is too long (" + std::to_string(len) + " samples)");
        n[b] = (int32_t)len;
        if (p.out_len(len) > longest) longest = p.out_len(len), longest_b = b;
    }
    if (y_stride < longest)
        return fail("vits_op_resample: y_stride = " + std::to_string(y_stride) + " is shorter than the longest output row (row " + std::to_string(longest_b) + ": " +
                    std::to_string(n[longest_b]) + " samples in, " + std::to_string(longest) + " out)");
    if (p.L == 1 && p.M == 1) {  // equal rates copy
        for (int b = 0; b < batch; ++b) std::memcpy(y + (size_t)b * y_stride, x + (size_t)b * x_stride, sizeof(float) * (size_t)n[b]);
        return 0;
    }
    const std::vector<float> ht = taps_kl(p);
    const size_t ny = (size_t)batch * y_stride * 4;
    DevMem dx, dy, dh, dn;
    // (y goes up too: what lies behind a row's output samples must come back as it was)
    if (!dx.put(x, (size_t)batch * x_stride * 4) || !dy.put(y, ny) || !dh.put(ht.data(), ht.size() * 4) || !dn.put(n.data(), (size_t)batch * 4)) return -1;
    ResampleCall c;
    c.x = dx.f();
    c.x_stride = x_stride;
    c.lens = dn.i();
    c.y = dy.f();
    c.y_stride = y_stride;
    c.taps = dh.f();
    c.plan = p;
    c.batch = batch;
    c.max_range = longest;
    return finish(launch_resample(c, nullptr)) && dy.get(y, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_pitch(int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const float* ratios, float* y, int64_t y_stride, int64_t* n_out) {
    VITS_TRY
    if (batch <= 0 || !x || !ratios || !y || !n_out || x_stride <= 0 || y_stride <= 0) return fail("vits_op_pitch: null argument or empty batch");
    std::vector<int32_t> n(batch);
    int64_t longest = 0, longest_b = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t len = lens ? lens[b] : x_stride;
        if (len < 0 || len > x_stride) return fail("vits_op_pitch: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]");
        PitchPlan p;
        std::string err;
        if (!pitch_plan(ratios[b], len, p, err)) return fail("vits_op_pitch: row " + std::to_string(b) + ": " + err);
        n[b] = (int32_t)len;
        n_out[b] = p.n_out;
        if (p.n_out > longest) longest = p.n_out, longest_b = b;
    }
    if (y_stride < longest)
        return fail("vits_op_pitch: y_stride = " + std::to_string(y_stride) + " is shorter than the longest output row (row " + std::to_string(longest_b) + ": " +
                    std::to_string(n[longest_b]) + " samples in, " + std::to_string(longest) + " out)");
    // the rows at the caller's own stride and at the caller's own alignment within 16 bytes (so that a test reaches the kernel's unaligned loads), 0xFF bytes
    // behind every length
    const size_t off = ((uintptr_t)x & 15) / 4;
    std::vector<float> hx((size_t)batch * x_stride + 4);
    std::memset(hx.data(), 0xFF, hx.size() * 4);
    for (int b = 0; b < batch; ++b) std::memcpy(&hx[off + (size_t)b * x_stride], x + (size_t)b * x_stride, sizeof(float) * (size_t)n[b]);
    const std::vector<float> gd = pitch_table_pairs();
    const size_t ny = (size_t)batch * y_stride * 4;
    DevMem dx, dy, dt, dn, dr;
    if (!dx.put(hx.data(), hx.size() * 4) || !dy.fill(ny, g_op_out_fill) || !dt.put(gd.data(), gd.size() * 4) || !dn.put(n.data(), (size_t)batch * 4) ||
        !dr.put(ratios, (size_t)batch * 4))
        return -1;
    PitchCall c;
    c.x = dx.f() + off;
    c.x_stride = x_stride;
    c.lens = dn.i();
    c.ratios = dr.f();
    c.y = dy.f();
    c.y_stride = y_stride;
    c.table = dt.f();
    c.batch = batch;
    c.max_out = longest;
    return finish(launch_pitch(c, nullptr)) && dy.get(y, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_tempo(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const float* tempos, float* y, int64_t y_stride,
                           int64_t* n_out, int32_t* offsets, int64_t offsets_stride) {
    VITS_TRY
    if (batch <= 0 || !x || !tempos || !y || !n_out || x_stride <= 0 || y_stride <= 0 || (offsets && offsets_stride <= 0))
        return fail("vits_op_tempo: null argument or empty batch");
    std::vector<int32_t> n(batch);
    int64_t longest = 0, longest_b = 0, most = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t len = lens ? lens[b] : x_stride;
        if (len < 0 || len > x_stride) return fail("vits_op_tempo: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]");
        TempoPlan p;
        std::string err;
        if (!tempo_plan(rate, tempos[b], len, p, err)) return fail("vits_op_tempo: row " + std::to_string(b) + ": " + err);
        n[b] = (int32_t)len;
        n_out[b] = p.n_out;
        most = std::max(most, p.F);
        if (p.n_out > longest) longest = p.n_out, longest_b = b;
    }
    if (y_stride < longest)
        return fail("vits_op_tempo: y_stride = " + std::to_string(y_stride) + " is shorter than the longest output row (row " + std::to_string(longest_b) + ": " +
                    std::to_string(n[longest_b]) + " samples in, " + std::to_string(longest) + " out)");
    if (offsets && offsets_stride < most)
        return fail("vits_op_tempo: offsets_stride = " + std::to_string(offsets_stride) + " is below the largest segment count (" + std::to_string(most) + ")");
    // the rows of x and y at the caller's own strides and at the caller's own alignment within 16 bytes (so that a test reaches the unaligned path), 0xFF
    // bytes behind every length of x, the fill byte all over y, the starts and the offsets
    const size_t offx = ((uintptr_t)x & 15) / 4, offy = ((uintptr_t)y & 15) / 4;
    std::vector<float> hx((size_t)batch * x_stride + 4);
    std::memset(hx.data(), 0xFF, hx.size() * 4);
    for (int b = 0; b < batch; ++b) std::memcpy(&hx[offx + (size_t)b * x_stride], x + (size_t)b * x_stride, sizeof(float) * (size_t)n[b]);
    const size_t ny = (size_t)batch * y_stride * 4, nof = offsets ? (size_t)batch * offsets_stride * 4 : 0;
    const int64_t ss = most + 1;
    DevMem dx, dy, ds, dof, dn, dq;
    if (!dx.put(hx.data(), hx.size() * 4) || !dy.fill(ny + 16, g_op_out_fill) || !ds.fill((size_t)batch * ss * 4, g_op_out_fill) || (offsets && !dof.fill(nof, g_op_out_fill)) ||
        !dn.put(n.data(), (size_t)batch * 4) || !dq.put(tempos, (size_t)batch * 4))
        return -1;
    TempoCall c;
    c.x = dx.f() + offx;
    c.x_stride = x_stride;
    c.lens = dn.i();
    c.tempos = dq.f();
    c.rate = rate;
    c.starts = ds.i();
    c.starts_stride = ss;
    c.offsets = offsets ? dof.i() : nullptr;
    c.offsets_stride = offsets_stride;
    c.y = dy.f() + offy;
    c.y_stride = y_stride;
    c.batch = batch;
    c.max_out = longest;
    hipError_t e = launch_tempo_search(c, nullptr);
    if (e == hipSuccess) e = launch_tempo_ola(c, nullptr);
    return finish(e) && DevMem::ok(hipMemcpy(y, c.y, ny, hipMemcpyDeviceToHost), "copy back failed") && (!offsets || dof.get(offsets, nof)) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_level(const vits_level_desc* d, const float* x, const int64_t* lens, float* y, float* levels) {
    VITS_TRY
    if (!d || !x || !levels || d->batch <= 0 || d->x_stride <= 0 || (y && d->y_stride <= 0)) return fail("vits_op_level: null argument or empty batch");
    if (d->kind == VITS_LEVEL_NONE) return fail("vits_op_level: VITS_LEVEL_NONE measures and applies nothing (use VITS_LEVEL_MEASURE)");
    LoudnessPlan plan;
    std::string err;
    if (!loudness_plan(d->rate, plan, err)) return fail("vits_op_level: " + err);
    if (!level_values_ok(d->kind, d->value_db, d->ceiling_db, err)) return fail("vits_op_level: " + err);
    const int B = d->batch;
    std::vector<int32_t> n;
    int64_t longest;
    if (!level_rows("vits_op_level", d, lens, y != nullptr, n, longest)) return -1;
    const int64_t xs = pcm_stride(longest);
    const size_t ny = (size_t)B * d->y_stride * 4;
    DevMem dx, dy, dlv, dscr, dn;
    // (y goes up too: what lies behind a row's samples must come back as it was)
    if (!stage_rows(dx, x, B, 1, d->x_stride, xs, n.data(), 0) || !dlv.fill((size_t)B * 4 * 4, 0) || !dscr.fill(level_scratch_bytes(B, longest, plan.S), 0) ||
        !dn.put(n.data(), (size_t)B * 4) || (y && !dy.put(y, ny)))
        return -1;
    hipError_t e = launch_level_measure(level_call(d, plan, dx, xs, dn, longest, dscr, dlv), nullptr);
    if (e == hipSuccess && y) {
        LevelScale sc;
        sc.x = dx.f();
        sc.x_stride = xs;
        sc.y = dy.f();
        sc.y_stride = d->y_stride;
        sc.lens = dn.i();
        sc.levels = dlv.f();
        sc.batch = B;
        sc.max_range = longest;
        e = launch_level_scale(sc, nullptr);
    }
    return finish(e) && dlv.get(levels, (size_t)B * 4 * 4) && (!y || dy.get(y, ny)) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_limit(const vits_limit_desc* ld, const float* x, const int64_t* lens, float* y, float* levels, float* limits) {
    VITS_TRY
    if (!ld || !x || !y || !levels || !limits || ld->level.batch <= 0 || ld->level.x_stride <= 0 || ld->level.y_stride <= 0)
        return fail("vits_op_limit: null argument or empty batch");
    const vits_level_desc* d = &ld->level;
    if (ld->mode != VITS_LIMIT_TRUE_PEAK)
        return fail(ld->mode == VITS_LIMIT_OFF ? "vits_op_limit: VITS_LIMIT_OFF limits nothing (use vits_op_level)" : "vits_op_limit: unknown mode " + std::to_string(ld->mode));
    if (d->kind == VITS_LEVEL_NONE || d->kind == VITS_LEVEL_MEASURE) return fail("vits_op_limit: VITS_LEVEL_NONE and VITS_LEVEL_MEASURE apply nothing: there is nothing to limit");
    LoudnessPlan plan;
    LimiterPlan lplan;
    std::string err;
    if (!limiter_plan(d->rate, lplan, err) || !loudness_plan(d->rate, plan, err)) return fail("vits_op_limit: " + err);
    if (!level_values_ok(d->kind, d->value_db, d->ceiling_db, err) || (d->kind == VITS_LEVEL_GAIN && !level_values_ok(VITS_LEVEL_LOUDNESS, 0.f, d->ceiling_db, err)))
        return fail("vits_op_limit: " + err);
    const int B = d->batch;
    std::vector<int32_t> n;
    int64_t longest;
    if (!level_rows("vits_op_limit", d, lens, true, n, longest)) return -1;
    const int64_t xs = pcm_stride(longest);
    const std::vector<float> ht = taps_kl(lplan.up);  // the 4x table
    const size_t ny = (size_t)B * d->y_stride * 4;
    DevMem dx, dy, dlv, dlm, dscr, dlscr, dt, dn;
    // (y goes up too: what lies behind a row's samples must come back as it was)
    if (!stage_rows(dx, x, B, 1, d->x_stride, xs, n.data(), 0) || !dlv.fill((size_t)B * 4 * 4, 0) || !dlm.fill((size_t)B * 4 * 4, 0) ||
        !dscr.fill(level_scratch_bytes(B, longest, plan.S), 0) || !dlscr.fill(limit_scratch_bytes(B, longest), 0) || !dt.put(ht.data(), ht.size() * 4) ||
        !dn.put(n.data(), (size_t)B * 4) || !dy.put(y, ny))
        return -1;
    const LevelCall c = level_call(d, plan, dx, xs, dn, longest, dscr, dlv);
    hipError_t e = launch_level_measure(c, nullptr);
    if (e == hipSuccess) {
        LimitCall mc;
        mc.x = dx.f();
        mc.x_stride = xs;
        mc.y = dy.f();
        mc.y_stride = d->y_stride;
        mc.lens = dn.i();
        mc.batch = B;
        mc.max_len = longest;
        mc.plan = lplan;
        mc.taps = dt.f();
        mc.scratch = dlscr.f();
        mc.kind = d->kind;
        mc.value_db = d->value_db;
        mc.gain = c.gain;
        mc.ceiling = (float)std::pow(10.0, (double)(d->kind == VITS_LEVEL_PEAK ? 0.f : d->ceiling_db) / 20.0);
        mc.levels = dlv.f();
        mc.limits = dlm.f();
        e = launch_limit(mc, nullptr);
    }
    return finish(e) && dlv.get(levels, (size_t)B * 4 * 4) && dlm.get(limits, (size_t)B * 4 * 4) && dy.get(y, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_edges(int32_t rate, const vits_edges_desc* desc, int32_t batch, const float* x, int64_t x_stride, const int32_t* lens, float* y, int64_t y_stride,
                           int32_t* lens_out, int64_t* rows) {
    VITS_TRY
    if (!desc || !x || !lens || !y || !lens_out || !rows || batch <= 0 || x_stride <= 0 || y_stride <= 0) return fail("vits_op_edges: null argument or empty batch");
    EdgesPlan plan;
    std::string err;
    if (!edges_plan(rate, *desc, plan, err)) return fail("vits_op_edges: " + err);
    if (plan.mode == VITS_EDGES_OFF) return fail("vits_op_edges: VITS_EDGES_OFF delivers the rows as they are: there is nothing to run");
    if (batch > 65535) return fail("vits_op_edges: more than 65535 rows");
    if (x == y) return fail("vits_op_edges: y must not be x");
    // (the one host read: the grids, the scratch and the y_stride check need the longest row)
    std::vector<int32_t> n((size_t)batch);
    if (hipMemcpy(n.data(), lens, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost) != hipSuccess) return fail("vits_op_edges: reading lens from the device failed");
    int64_t longest = 0;
    for (int b = 0; b < batch; ++b) {
        if (n[b] < 0 || n[b] > x_stride) return fail("vits_op_edges: lens[" + std::to_string(b) + "] = " + std::to_string(n[b]) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]");
        if (n[b] > kEdgesMaxLen) return fail("vits_op_edges: row " + std::to_string(b) + " is too long (" + std::to_string(n[b]) + " samples)");
        longest = std::max<int64_t>(longest, n[b]);
    }
    if (y_stride < plan.bound(longest))
        return fail("vits_op_edges: y_stride = " + std::to_string(y_stride) + " is below the largest bound (" + std::to_string(longest) + " samples + Pl + Pt = " +
                    std::to_string(plan.bound(longest)) + ")");
    const std::vector<float> fades = edges_fades(plan);
    DevMem dscr, df;
    if (!dscr.fill(edges_scratch_bytes(batch, longest, plan.W), 0) || (!fades.empty() && !df.put(fades.data(), fades.size() * 4))) return -1;
    EdgesCall c;
    c.x = x;
    c.x_stride = x_stride;
    c.lens = lens;
    c.y = y;
    c.y_stride = y_stride;
    c.batch = batch;
    c.max_len = longest;
    c.plan = plan;
    c.fades = df.f();
    c.scratch = dscr.f();
    c.lens_out = lens_out;
    c.rows = rows;
    hipError_t e = launch_edges_window(c, nullptr);
    if (e == hipSuccess) e = launch_edges_bounds(c, nullptr);
    if (e == hipSuccess) e = launch_edges_apply(c, nullptr);
    return finish(e) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_join(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int32_t* lens, const int32_t* track, const float* gap_ms, float* y,
                          int64_t y_stride, int32_t* track_lens_out, int64_t* offsets_out) {
    VITS_TRY
    if (!x || !lens || !y || !track_lens_out || !offsets_out || batch <= 0 || x_stride <= 0 || y_stride <= 0) return fail("vits_op_join: null argument or empty batch");
    JoinPlan plan;
    std::string err;
    if (!join_plan(rate, batch, track, gap_ms, plan, err)) return fail("vits_op_join: " + err);
    std::vector<int64_t> ub((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        if (lens[b] < 0 || lens[b] > x_stride) return fail("vits_op_join: lens[" + std::to_string(b) + "] = " + std::to_string(lens[b]) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]");
        ub[(size_t)b] = lens[b];
    }
    if (!join_bounds(plan, ub.data(), err)) return fail("vits_op_join: " + err);
    if (y_stride < plan.max_bound) return fail("vits_op_join: y_stride = " + std::to_string(y_stride) + " is below the largest track bound (" + std::to_string(plan.max_bound) + " samples)");
    const std::vector<int64_t> table = join_table(plan);
    const int G = plan.tracks;
    const size_t ny = (size_t)G * y_stride * 4;
    DevMem dx, dy, dn, dt, drows, dtl;
    // (y goes up too: what lies behind a track's bound must come back as it was)
    if (!dx.put(x, (size_t)batch * x_stride * 4) || !dy.put(y, ny) || !dn.put(lens, (size_t)batch * 4) || !dt.put(table.data(), table.size() * 8) ||
        !drows.fill((size_t)batch * 2 * 8, 0) || !dtl.fill((size_t)G * 4, 0))
        return -1;
    JoinCall c;
    c.plan = &plan;
    c.x = dx.f();
    c.x_stride = x_stride;
    c.lens = dn.i();
    c.y = dy.f();
    c.y_stride = y_stride;
    c.table = static_cast<const int64_t*>(dt.p);
    c.rows = static_cast<int64_t*>(drows.p);
    c.track_lens = dtl.i();
    hipError_t e = launch_join_offsets(c, nullptr);
    if (e == hipSuccess) e = launch_join_apply(c, nullptr);
    return finish(e) && dy.get(y, ny) && drows.get(offsets_out, (size_t)batch * 2 * 8) && dtl.get(track_lens_out, (size_t)G * 4) ? 0 : -1;
    VITS_CATCH(-1)
}
