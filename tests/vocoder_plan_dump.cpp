// vocoder_plan_dump — prints the schedule of the vocoder's stages (vits.cpp_amd/csrc/vocoder_plan.cpp) over a fixed sweep of stages, batches, lengths, arithmetic
// modes and knob sets as text, one line per case: tests/test_vocoder_plan_host.py compares the output with tests/golden/vocoder_plan_table.txt byte for byte.
// Links vocoder_plan.o, conv_plan.o and launch_plan.o alone (csrc/Makefile, target vocoder_plan_dump): the schedule touches no device.
//
// A line '## name' opens a knob set, a line '@ stage arith planes prof aligned' names the context of the case lines behind it (arith: 0 fp32, 1 f16, 2 bf16,
// 3 fp32 on split operands; planes: the call has the buffers of the split planes; prof: the per-kernel profiler is on; aligned: the fused fp32 kernels' pointer
// and stride test). A case line is 'B frames : fields', B utterances of `frames` frames each; the stage's longest utterance is frames x the stage's upsampling.
//   16-bit layout   kernels all_block par sum3 longest_first group3 lat3
//   fp32 layout     kernels any_split grouped par sum3 lcopy [the kernels Engine::plan_tile_maps plans lists for: exact fp32 only, and not compared]
//   stage 'pre'     pre_lat (the window's conv_pre; `frames` is the window's longest utterance)
// kernels: one digit per resblock, 0 two launches per pair, 1 the same on split operands, 2 fused pairs, 3 the whole-resblock kernel.
// The default knob set: exact fp32 and f16 (planes 1, prof 0, aligned 1) print every case, every other context the cases whose line differs from its parent
// context's (parent(), below); the model's own stages walk the whole grid, the stages the fused kernels refuse a thinner one. Every other knob set prints, on the
// model's stages and the thinner grid (f32, f16 and split with planes 1, aligned 1), the cases whose line differs from the default set's.
// Exits non-zero if a plan names a fused kernel whose own *_supported predicate refuses the shape.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/vocoder_plan.h"

using namespace vits;

static float g_dummy[8];  // (pointers are only tested for null)
static uint16_t g_dummy16[8];

// a resblock conv as conv_plan_dump.cpp's make_conv builds it
static PackedConv make_conv(int C, int k) {
    PackedConv w;
    const ConvPackDims d = conv_pack_dims(C, C, k, EPI_STD, 0);
    w.cin = w.cout = C, w.kt = d.kt, w.rows = d.rows, w.mtiles = d.mtiles, w.mtiles_used = d.mtiles_used, w.nchunks = d.nchunks;
    w.epi = EPI_STD;
    w.wp = g_dummy, w.bias = g_dummy, w.wp16 = g_dummy16;
    if (conv_lat16_candidate(EPI_STD, d.kt, C)) w.wp_l16 = g_dummy;
    if (conv_split_candidate(EPI_STD, d.kt, C, C)) w.wps = g_dummy16;
    return w;
}
static ResBlockW make_rb(int C, int k, std::vector<int> dil = {1, 3, 5}) {
    ResBlockW R;
    R.k = k, R.dil = dil;
    for (size_t d = 0; d < dil.size(); ++d) R.c1.push_back(make_conv(C, k)), R.c2.push_back(make_conv(C, k));
    return R;
}
struct Stage {
    const char* name;
    UpStageW U;
    int mult;  // output columns per frame (VITS-english: upsampling 8, 8, 2, 2)
    bool model;  // a stage of the model itself: the knob sets walk these
};
static int mult_of(int C) { return C == 256 ? 8 : C == 128 ? 64 : C == 64 ? 128 : 256; }
static std::vector<Stage> stages() {
    std::vector<Stage> v;
    auto add = [&](const char* name, int C, std::vector<int> ks, bool model = false) -> UpStageW& {
        Stage s{name, UpStageW(), mult_of(C), model};
        s.U.channels = C, s.U.stride = C >= 128 ? 8 : 2, s.U.k = 2 * s.U.stride;
        for (int k : ks) s.U.rbs.push_back(make_rb(C, k));
        v.push_back(s);
        return v.back().U;
    };
    for (int C : {256, 128, 64, 32}) add(C == 256 ? "c256" : C == 128 ? "c128" : C == 64 ? "c64" : "c32", C, {3, 7, 11}, true);
    // what the fused kernels refuse
    add("c64.nk1", 64, {3}), add("c64.nk2", 64, {3, 7}), add("c256.nk2", 256, {3, 7}), add("c32.nk4", 32, {3, 7, 11, 3});
    add("c64.dil132", 64, {3, 7, 11}).rbs[1] = make_rb(64, 7, {1, 3, 2});
    add("c256.dil13", 256, {3, 7, 11}).rbs[2] = make_rb(256, 11, {1, 3});
    add("c128.dil13x3", 128, {3, 7, 11}).rbs = {make_rb(128, 3, {1, 3}), make_rb(128, 7, {1, 3}), make_rb(128, 11, {1, 3})};
    add("c64.k5", 64, {3, 5, 11}), add("c128.k5", 128, {3, 5, 11});
    add("c32.nobias", 32, {3, 7, 11}).rbs[0].c2[1].bias = nullptr;
    add("c32.nobias11", 32, {3, 7, 11}).rbs[2].c1[0].bias = nullptr;
    add("c128.nobias", 128, {3, 7, 11}).rbs[1].c1[2].bias = nullptr;
    add("c32.nowp16", 32, {3, 7, 11}).rbs[1].c1[0].wp16 = nullptr;
    add("c64.nowp16.11", 64, {3, 7, 11}).rbs[2].c2[2].wp16 = nullptr;
    add("c256.nowp16", 256, {3, 7, 11}).rbs[0].c1[1].wp16 = nullptr;
    add("c64.nowp", 64, {3, 7, 11}).rbs[0].c1[0].wp = nullptr;
    add("c128.nowps", 128, {3, 7, 11}).rbs[1].c2[0].wps = nullptr;
    add("c256.nowps", 256, {3, 7, 11}).rbs[2].c1[2].wps = nullptr;
    return v;
}

struct Grid {
    int B, f;
    bool thin;  // the knob sets other than the default walk these
};
static const Grid kGrid[] = {
    // the batches of 128-id utterances
    {1, 290, true}, {2, 290, true}, {3, 290, false}, {4, 290, true}, {8, 290, true}, {16, 290, false}, {64, 290, true},
    // both sides of the frame thresholds: 600 (16-bit: side by side below), 1300 (16-bit: one stream up to it), 2000 (fp32: side by side below)
    {1, 599, true}, {1, 600, true}, {1, 1300, true}, {1, 1301, true}, {1, 1999, true}, {1, 2000, true}, {2, 299, false}, {2, 300, false}, {3, 666, false}, {3, 667, false},
    // conv16_lat_kernel's tile caps: C = 256, 2048 tiles = 8192 columns; C = 128 (VITS_LAT16H_MAX_TILES_C128=4096), 4096 tiles = 32768 columns
    {1, 1024, true}, {1, 1025, true}, {4, 256, false}, {5, 256, false}, {1, 512, true}, {1, 513, true},
    // the grouped whole-resblock launch's 3072 blocks of 184 columns (reached side by side only under VITS_RB16_SERIAL_MIN_FRAMES)
    {1, 2208, true}, {1, 2209, true}, {64, 69, true}, {64, 70, true},
    // the fp32 grouped launch's 128 x 128 tile: small grids step down from it
    {1, 20, true}, {1, 100, false},
};
// conv_pre (192 -> 512 channels, k = 7): 2048 tiles = 128 column tiles of 32
static const Grid kPreGrid[] = {{1, 290, true}, {2, 290, true}, {4, 290, true}, {8, 290, true}, {64, 290, true}, {1, 4096, true}, {1, 4097, true}, {4, 1024, true}, {5, 1024, true}};

struct KnobSet {
    const char* name;
    VocPolicy p;
    KernelKnobs k;
    bool no_fuse16 = false, no_group16 = false;  // VITS_NO_FUSE16; VITS_NO_GROUP16: the 16-bit modes through the fp32 layout (converter path)
};
static std::vector<KnobSet> knob_sets() {
    std::vector<KnobSet> v;
    auto add = [&](const char* name, auto set) {
        KnobSet s{name, VocPolicy(), KernelKnobs()};  // (the defaults of the structs, not of the environment)
        set(s);
        v.push_back(s);
    };
    add("default", [](KnobSet&) {});
    add("rb_streams=1", [](KnobSet& s) { s.p.rb_streams = 1; });
    add("rb_group_always", [](KnobSet& s) { s.p.rb_group_always = true; });
    add("no_rb_group", [](KnobSet& s) { s.p.no_rb_group = true; });
    add("no_rbblock16", [](KnobSet& s) { s.p.no_rbblock16 = true; });
    add("no_fuse16", [](KnobSet& s) { s.no_fuse16 = true; });
    add("no_group16", [](KnobSet& s) { s.no_group16 = true; });
    add("no_fuse32", [](KnobSet& s) { s.p.no_fuse32 = true; });
    add("no_rbblock32", [](KnobSet& s) { s.p.no_rbblock32 = true; });
    add("rb16_serial_max_frames=2500", [](KnobSet& s) { s.p.rb16_serial_max_frames = 2500; });
    add("rb16_serial_min_frames=1000000", [](KnobSet& s) { s.p.rb16_serial_min_frames = 1000000; });
    add("rb16_serial_min_frames=0", [](KnobSet& s) { s.p.rb16_serial_min_frames = 0; });
    add("rb32_sum3_max_frames=0", [](KnobSet& s) { s.p.rb32_sum3_max_frames = 0; });
    add("lrelu_copy_minc=1000", [](KnobSet& s) { s.p.lrelu_copy_minc = 1000; });
    add("no_rb_sum3", [](KnobSet& s) { s.k.no_rb_sum3 = true; });
    add("no_rb_sum3_f32", [](KnobSet& s) { s.k.no_rb_sum3_f32 = true; });
    add("rb_sum3_block_only", [](KnobSet& s) { s.k.rb_sum3_block_only = true; });
    add("rb_sum3_in_order", [](KnobSet& s) { s.k.rb_sum3_in_order = true; });
    add("no_rbb_group3", [](KnobSet& s) { s.k.no_rbb_group3 = true; });
    add("no_rbb_group3_c64", [](KnobSet& s) { s.k.no_rbb_group3_c64 = true; });
    add("no_lat16h", [](KnobSet& s) { s.k.no_lat16h = true; });
    add("no_lat16h_group", [](KnobSet& s) { s.k.no_lat16h_group = true; });
    add("no_lat16h_pre", [](KnobSet& s) { s.k.no_lat16h_pre = true; });
    add("lat16h_max_tiles=1024", [](KnobSet& s) { s.k.lat16h_max_tiles = 1024; });
    add("lat16h_max_tiles_c128=4096", [](KnobSet& s) { s.k.lat16h_max_tiles_c128 = 4096; });
    add("fuse16_maxc=64", [](KnobSet& s) { s.k.fuse16_maxc = 64; });
    add("fuse32_c128=0", [](KnobSet& s) { s.k.fuse32_c128 = false; });
    add("rbb_c128=0", [](KnobSet& s) { s.k.rbb_c128 = false; });
    add("rbb_c64k11=1", [](KnobSet& s) { s.k.rbb_c64k11 = 1; });
    add("rbb_c64k11=0", [](KnobSet& s) { s.k.rbb_c64k11 = 0; });
    add("tile128=0", [](KnobSet& s) { s.k.tile128 = 0; });
    // the combinations the GPU tests run
    add("rb_streams=1+rb_group_always", [](KnobSet& s) { s.p.rb_streams = 1, s.p.rb_group_always = true; });
    add("no_rbblock16+no_fuse16", [](KnobSet& s) { s.p.no_rbblock16 = true, s.no_fuse16 = true; });
    add("no_fuse32+no_rbblock32", [](KnobSet& s) { s.p.no_fuse32 = true, s.p.no_rbblock32 = true; });
    add("no_rb_sum3+no_rb_sum3_f32", [](KnobSet& s) { s.k.no_rb_sum3 = true, s.k.no_rb_sum3_f32 = true; });
    add("rb16_serial_min_frames=1000000+no_rbb_group3", [](KnobSet& s) { s.p.rb16_serial_min_frames = 1000000, s.k.no_rbb_group3 = true; });
    add("rb16_serial_min_frames=1000000+no_lat16h", [](KnobSet& s) { s.p.rb16_serial_min_frames = 1000000, s.k.no_lat16h = true; });
    add("no_rbblock32+lrelu_copy_minc=1000", [](KnobSet& s) { s.p.no_rbblock32 = true, s.p.lrelu_copy_minc = 1000; });
    return v;
}

// the context of a case as Engine::voc_policy fills it
struct Ctx {
    int arith;  // 0 fp32, 1 f16, 2 bf16, 3 fp32 on split operands
    bool planes, prof, aligned;
};
static int key(const Ctx& c) { return c.arith * 8 + c.planes * 4 + c.prof * 2 + c.aligned; }
// The context whose lines stand for this one's where they are equal (false: none, the context prints every case): bf16 reads f16's, the split arithmetic exact
// fp32's, a call without the split planes' buffers the one with them, then unaligned buffers aligned ones, then the profiler's schedule the plain one
static bool parent(Ctx& c) {
    if (c.arith == 2) c.arith = 1;
    else if (c.arith == 3) c.arith = 0, c.planes = true;
    else if (!c.planes) c.planes = true;
    else if (!c.aligned) c.aligned = true;
    else if (c.prof) c.prof = false;
    else return false;
    return true;
}
static bool layout16(const Ctx& c, const KnobSet& ks) { return (c.arith == 1 || c.arith == 2) && !ks.no_group16; }
static VocPolicy policy(const Ctx& c, const KnobSet& ks) {
    VocPolicy p = ks.p;
    p.prof_on = c.prof;
    p.fuse16 = layout16(c, ks) && !ks.no_fuse16;
    p.arith_now = c.arith == 1 ? VITS_ARITH_F16 : c.arith == 2 ? VITS_ARITH_BF16 : VITS_ARITH_F32;
    p.split_on = c.arith == 3;
    p.split_planes = c.planes;
    p.aligned = c.aligned;
    return p;
}

// ---- the case lines ------------------------------------------------------------------------------------------------------------------------------------------
static int g_refused = 0;
static void check(bool named, bool supported, const char* what, const Stage& s, int B, int t_out) {
    if (!named || supported) return;
    std::fprintf(stderr, "%s: the plan of stage %s, B %d, t_out %d names a kernel that refuses it\n", what, s.name, B, t_out);
    ++g_refused;
}
static std::string digits(const RbKernel* rb, size_t nk) {
    std::string d;
    for (size_t j = 0; j < nk && j < (size_t)kVocRb; ++j) d += (char)('0' + (int)rb[j]);
    return d;
}
static std::string case16(const Stage& s, int B, int t_out, int64_t frames, const VocPolicy& p) {
    const UpStageW& U = s.U;
    const int C = U.channels;
    const VocStage16Plan pl = plan_voc_stage16(U, B, t_out, frames, p);
    std::string kernels = digits(pl.rb, U.rbs.size());
    for (size_t j = kVocRb; j < U.rbs.size(); ++j) kernels += (char)('0' + (int)rb_kernel16_of(pl, U, j, B, t_out, p));
    for (size_t j = 0; j < U.rbs.size(); ++j) {
        const ResBlockW& R = U.rbs[j];
        const RbKernel k = rb_kernel16_of(pl, U, j, B, t_out, p);
        check(k == RbKernel::Block, rbblock16_supported(C, R.k, R.dil.data(), (int)R.dil.size(), B, t_out), "rbblock16", s, B, t_out);
        for (int d : R.dil) check(k == RbKernel::Pairs, rbpair16_supported(C, R.k, d), "rbpair16", s, B, t_out);
        for (int d : R.dil) check(pl.lat3, conv16_lat_shape_ok(C, R.k, d, B, t_out) && conv16_lat_shape_ok(C, R.k, 1, B, t_out), "conv16_lat_group", s, B, t_out);
    }
    if (pl.group3) {
        const int kts[3] = {U.rbs[0].k, U.rbs[1].k, U.rbs[2].k};
        check(true, rbblock16_group3_supported(C, kts, B, t_out), "rbblock16_group3", s, B, t_out);
    }
    char b[64];
    std::snprintf(b, sizeof(b), "%s %d%d%d%d%d%d", kernels.c_str(), pl.all_block, pl.par, pl.sum3, pl.longest_first, pl.group3, pl.lat3);
    return b;
}
static std::string case32(const Stage& s, int B, int t_out, int64_t frames, const VocPolicy& p) {
    const UpStageW& U = s.U;
    const int C = U.channels;
    const VocStage32Plan pl = plan_voc_stage32(U, B, t_out, frames, p);
    std::string kernels;
    for (size_t j = 0; j < U.rbs.size(); ++j) {
        const ResBlockW& R = U.rbs[j];
        const RbKernel k = pl.kernel_of(j);
        kernels += (char)('0' + (int)k);
        check(k == RbKernel::Block, rbblock32_supported(C, R.k, R.dil.data(), (int)R.dil.size()), "rbblock32", s, B, t_out);
        for (size_t d = 0; d < R.dil.size(); ++d) {
            check(k >= RbKernel::Pairs, rbpair32_supported(C, R.k, R.dil[d]), "rbpair32", s, B, t_out);
            check(k == RbKernel::Split, conv_split_supported(R.c1[d], R.dil[d]) && conv_split_supported(R.c2[d], 1), "conv_split", s, B, t_out);
            check(pl.grouped && !pl.fused(j), conv_group_supported(R.c1[d], R.dil[d]) && conv_group_supported(R.c2[d], 1), "conv_group", s, B, t_out);
        }
    }
    char b[64];
    std::snprintf(b, sizeof(b), "%s %d%d%d%d%d", kernels.c_str(), pl.any_split, pl.grouped, pl.par, pl.sum3, pl.lcopy);
    return b;
}
// the kernels Engine::plan_tile_maps plans lists for: the same planner before the call's buffers are laid out (aligned: true)
static std::string lists32(const Stage& s, int B, int t_out, int64_t frames, VocPolicy p) {
    p.aligned = true;
    const VocStage32Plan tm = plan_voc_stage32(s.U, B, t_out, frames, p);
    std::string lists = " ";
    for (size_t j = 0; j < s.U.rbs.size(); ++j) lists += (char)('0' + (int)tm.kernel_of(j));
    return lists;
}
static std::string case_pre(int B, int Lw, const VocPolicy& p) {
    PackedConv pre;
    const ConvPackDims d = conv_pack_dims(512, 192, 7, EPI_STD, 0);
    pre.cin = 192, pre.cout = 512, pre.kt = d.kt, pre.rows = d.rows, pre.mtiles = d.mtiles, pre.mtiles_used = d.mtiles_used, pre.nchunks = d.nchunks;
    pre.wp = g_dummy, pre.bias = g_dummy, pre.wp16 = g_dummy16;
    return std::to_string((int)plan_voc_pre_lat(pre, 192, B, Lw, p));
}

int main() {
    const std::vector<Stage> S = stages();
    std::vector<Ctx> ctxs;
    for (int arith : {0, 1, 2, 3})
        for (bool planes : {true, false})
            for (bool prof : {false, true})
                for (bool aligned : {true, false}) ctxs.push_back({arith, planes, prof, aligned});
    std::puts("# @ stage arith planes prof aligned");
    std::puts("# B frames : kernels {all_block par sum3 longest_first group3 lat3}                      (16-bit layout)");
    std::puts("# B frames : kernels {any_split grouped par sum3 lcopy} [kernels of the tile lists]      (fp32 layout)");
    std::puts("# B frames : pre_lat                                                                     (stage pre)");
    std::map<std::string, std::string> base;  // the default knob set's line per (stage, context, case)
    for (const KnobSet& ks : knob_sets()) {
        KernelKnobsScope scope(&ks.k);
        const bool def = base.empty();
        std::printf("## %s\n", ks.name);
        for (size_t si = 0; si <= S.size(); ++si) {  // (si == S.size(): the window's conv_pre)
            const bool pre = si == S.size();
            if (!def && !pre && !S[si].model) continue;
            std::map<std::string, std::string> lines[32];  // the default set's line per context and case
            for (const Ctx& c : ctxs) {
                if (!def && (!c.planes || !c.aligned || c.arith == 2)) continue;
                if (pre && (!layout16(c, ks) || !c.planes || !c.aligned)) continue;
                const VocPolicy p = policy(c, ks);
                const bool l16 = layout16(c, ks), thin = !def || (!pre && !S[si].model);
                bool named = false;
                auto emit = [&](Grid g, const std::string& fields, const std::string& lists = "") {  // (the lists follow the fields: they are not compared)
                    const std::string cs = std::to_string(g.B) + " " + std::to_string(g.f);
                    std::string& b = base[std::to_string(si) + "/" + std::to_string(key(c)) + "/" + cs];
                    if (def) {
                        b = lines[key(c)][cs] = fields;
                        Ctx up = c;
                        if (parent(up) && lines[key(up)][cs] == fields) return;
                    } else if (b == fields) {
                        return;
                    }
                    if (!named) std::printf("@ %s %d %d %d %d\n", pre ? "pre" : S[si].name, c.arith, c.planes, c.prof, c.aligned);
                    named = true;
                    std::printf("%s : %s%s\n", cs.c_str(), fields.c_str(), lists.c_str());
                };
                if (pre) {
                    for (Grid g : kPreGrid) emit(g, case_pre(g.B, g.f, p));
                    continue;
                }
                for (Grid g : kGrid) {
                    if (thin && !g.thin) continue;
                    const int t_out = g.f * S[si].mult;
                    const int64_t frames = (int64_t)g.B * g.f;
                    if (l16) emit(g, case16(S[si], g.B, t_out, frames, p));
                    else emit(g, case32(S[si], g.B, t_out, frames, p), c.arith == 0 ? lists32(S[si], g.B, t_out, frames, p) : "");
                }
            }
        }
    }
    return g_refused ? 1 : 0;
}
