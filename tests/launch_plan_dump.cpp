// launch_plan_dump — prints the launch policy of the fused kernels (vits.cpp_amd/csrc/launch_plan.cpp) over a fixed sweep of shapes, grids and knob
// sets as text, one line per case: tests/test_launch_plan_host.py compares the output with tests/golden/launch_plan_table.txt byte for byte.
// Links launch_plan.o alone (csrc/Makefile, target launch_plan_dump): the policy touches no device.
//
// Lines: `<family> <case> : <fields>`; the header lines starting with '#' name the fields. `kernel` is the instantiation the launcher takes, with the operand
// type argument at `false` (f16). The default knob set prints every case; every other knob set prints the cases whose line differs from the default one.
// Exits non-zero if a plan marked launchable names an instantiation that the launchers' own predicates (rbpair16_exists and its kin) say does not exist.
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/launch_plan.h"

using namespace vits;

static std::string fmt(const char* f, ...) {
    char b[256];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}
static const char* tf(bool v) { return v ? "true" : "false"; }
static std::string grid_fields(const LaunchGrid& l) { return fmt("%d %d %d %d %zu", l.gx, l.gy, l.gz, l.block, l.lds); }
static int g_missing = 0;
static void check_exists(bool ok, bool exists, const std::string& what) {
    if (!ok || exists) return;
    std::fprintf(stderr, "no such instantiation: %s\n", what.c_str());
    ++g_missing;
}
static uint16_t g_dummy16[8];
static float g_dummy[8];

// ---- one line per case ------------------------------------------------------------------------------------------------------------------
static std::string row_rbpair16(int C, int k, int d, int T, int B) {
    const RbPair16Plan p = plan_rbpair16(C, k, d, B, T);
    const std::string sup = fmt("%d", rbpair16_supported(C, k, d));
    if (!p.ok) return sup + " 0 -";
    const std::string kernel = fmt("rbpair16_kernel<%d, %d, %d, %d, false, %s>", k, d, C, p.nr, tf(rbpair16_geom(k, d, C, p.nr).rows));
    check_exists(true, rbpair16_exists(k, d, C, p.nr), kernel);
    return sup + " 1 " + kernel + " | " + grid_fields(p);
}
static std::string row_rbblock16(int C, int k, int T, int B) {
    const int d135[3] = {1, 3, 5}, d132[3] = {1, 3, 2};
    const RbBlock16Plan p = plan_rbblock16(C, k, B, T);
    const std::string sup = fmt("%d%d%d", rbblock16_supported(C, k, d135, 3, B, T), rbblock16_supported(C, k, d132, 3, B, T), rbblock16_supported(C, k, d135, 2, B, T));
    if (!p.ok) return sup + " 0 -";
    const std::string kernel = fmt("rbblock16_kernel<%d, %d, %d, %d, %d, 1, 3, 5, false, %s>", k, C, p.tile.nstrip, p.tile.nrw, p.tile.mrw, tf(p.nt > 1));
    check_exists(true, rbblock16_exists(k, C), kernel);
    return sup + " 1 " + kernel + fmt(" nt %d | ", p.nt) + grid_fields(p);
}
static std::string row_group3(int C, int T, int B) {
    const int kts[3] = {3, 7, 11}, other[3] = {3, 7, 7};
    const LaunchGrid p = plan_rbblock16_group3(C, kts, B, T);
    const std::string sup = fmt("%d%d", rbblock16_group3_supported(C, kts, B, T), rbblock16_group3_supported(C, other, B, T));
    if (!p.ok) return sup + " 0 -";
    check_exists(true, rbblock16_group3_exists(C), "rbblock16_group3_kernel");
    return sup + " 1 " + fmt("rbblock16_group3_kernel<%d, false> | ", C) + grid_fields(p);
}
static std::string row_rbpair32(int C, int k, int d, int T, int B) {
    const LaunchGrid p = plan_rbpair32(C, k, d, B, T);
    const std::string sup = fmt("%d", rbpair32_supported(C, k, d));
    if (!p.ok) return sup + " 0 -";
    const std::string kernel = fmt("rbpair32_kernel<%d, %d, %d>", k, d, C);
    check_exists(true, rbpair32_exists(k, d, C), kernel);
    return sup + " 1 " + kernel + " | " + grid_fields(p);
}
static std::string row_rbblock32(int C, int k, int T, int B) {
    const int d135[3] = {1, 3, 5}, d132[3] = {1, 3, 2};
    const RbBlock32Plan p = plan_rbblock32(C, k, B, T);
    const std::string sup = fmt("%d%d", rbblock32_supported(C, k, d135, 3), rbblock32_supported(C, k, d132, 3));
    if (!p.ok) return sup + " 0 -";
    const std::string kernel = fmt("rbblock32_kernel<%d, %d>", C, p.nr);
    check_exists(true, p.nr != 0 && rbblock32_exists(C, p.nr), kernel);
    return sup + " 1 " + kernel + " | " + grid_fields(p);
}
static PackedConv make_convt(int cin, int cout, int stride, bool planes) {
    PackedConv w;
    w.cin = cin, w.cout = cout, w.kt = 2, w.rows = cout * stride, w.epi = EPI_CONVT, w.ct_stride = stride;
    w.mtiles_used = (w.rows + 31) / 32, w.mtiles = (w.mtiles_used + 3) / 4 * 4, w.nchunks = (cin + 31) / 32;
    w.wp = g_dummy, w.bias = g_dummy;
    if (planes) w.wp16 = g_dummy16;
    return w;
}
static std::string row_convt16(int cin, int cout, int stride, int T, int B) {
    const PackedConv w = make_convt(cin, cout, stride, true), w0 = make_convt(cin, cout, stride, false);
    const ConvT16Plan p = plan_convt16(w, B, T);
    const std::string sup = fmt("%d%d", convt16_stream_supported(w), convt16_stream_supported(w0));
    char tag[24] = "-";
    if (convt16_stream_supported(w)) convt16_stream_tag(w, tag, sizeof(tag));  // (as the engine asks: only where the streaming kernel is taken)
    if (!p.ok) return sup + " 0 " + tag + " -";
    const std::string kernel = p.lines_bn ? fmt("convt16_lines_kernel<%d, false>", p.lines_bn) : fmt("convt16_kernel<%d, %d, %d, false>", p.nr, p.csplit, p.rs);
    check_exists(true, convt16_exists(p.lines_bn, p.nr, p.csplit, p.rs), kernel);
    return sup + " 1 " + tag + " " + kernel + " | " + grid_fields(p);
}
static std::string row_wavenet(int hidden, int k, int d, int T, int B) {
    const WaveNetPlan p32 = plan_wavenet32(hidden, k, d, B, T), p16 = plan_wavenet16(hidden, k, d, B, T);
    if (!p32.ok && !p16.ok) return "0 0 -";
    check_exists(p16.ok, wavenet16_exists(p16.ncw), "wavenet16_kernel");
    return fmt("%d %d wavenet32_kernel<192, 5> | ", p32.ok, p16.ok) + grid_fields(p32) + fmt(" | wavenet16_kernel<192, 5, false, %d> | ", p16.ncw) + grid_fields(p16);
}
// (wide: the 48-frame blocks of ONE utterance of T frames; narrow: whether a launch of wide x B blocks runs on 16-frame blocks — the engine's chain split asks both)
static std::string row_flow(int hidden, int half, int k, int rate, int layers, int T, int B) {
    const FlowCouple16Plan p = plan_flow_couple16(hidden, half, k, rate, layers, B, T);
    const std::string tail = fmt(" | wide %d narrow %d", flow_wide_blocks(T), flow_couple16_narrow((int64_t)flow_wide_blocks(T) * B));
    if (!p.ok) return "0 -" + tail;
    const std::string kernel = fmt("flow_couple16_kernel<false, %d, %d>", p.ncw, p.nct);
    check_exists(true, flow_couple16_exists(p.ncw, p.nct), kernel);
    return "1 " + kernel + " | " + grid_fields(p) + tail;
}
static std::string row_attention(int heads, int hd, int w, int T, int B) {
    const AttentionPlan p = plan_rel_attention(B, heads, hd, T, w);
    if (!p.ok) return "0 -";
    const std::string kernel = p.mfma ? fmt("rel_attention_mfma_kernel<%d, %d, %s, %s>", p.nw, p.maxs, tf(p.sh), tf(p.lat)) : fmt("rel_attention_kernel<%d>", p.block);
    check_exists(true, p.mfma ? att_mfma_exists(p.nw, p.maxs, p.sh, p.lat) : att_valu_exists(p.block), kernel);
    return "1 " + kernel + " | " + grid_fields(p) + (p.mfma ? std::string(" | -") : fmt(" | vshift %d", p.vshift));
}
static std::string row_layer_norm(int C, int T, int B) {
    const LayerNormPlan p = plan_add_layer_norm(C, B, T);
    if (!p.ok) return "0 -";
    check_exists(true, p.tw == 32 || p.tw == 64, "add_layer_norm_kernel");
    return fmt("1 add_layer_norm_kernel<%d> | ", p.tw) + grid_fields(p);
}
static std::string row_depthwise(int C, int k, int d, int T, int B) {
    const LaunchGrid p = plan_dds_depthwise(C, k, d, B, T);
    return p.ok ? "1 | " + grid_fields(p) : std::string("0 -");
}
static PackedConv make_pointwise(int C) {
    PackedConv w;
    w.cin = w.cout = C, w.kt = 1, w.rows = C, w.epi = EPI_STD, w.nchunks = (C + 31) / 32, w.mtiles_used = (C + 31) / 32, w.mtiles = (w.mtiles_used + 3) / 4 * 4;
    w.wp = w.bias = w.wp_l16 = g_dummy, w.wp16 = g_dummy16;
    return w;
}
static std::string row_dds_layer(int C, int k, int d, int T, int B) {
    const PackedConv pw = make_pointwise(C);
    const DdsLayerPlan p = plan_dds_layer(C, k, d, B, T);
    const std::string sup = fmt("%d", dds_layer_supported(pw, C, k, d, 0));
    if (!p.ok) return sup + " 0 -";
    check_exists(true, p.m == 2 || p.m == 4 || p.m == 6 || p.m == 8, "dds_layer_kernel");
    return sup + fmt(" 1 dds_layer_kernel<0, %d> | ", p.m) + grid_fields(p);
}
// (grid_ok: the engine's rule for taking the latency kernel on this grid; the two launches: no head, and the H -> H 1x1 conv in front)
static std::string row_dds_lat(int C, int k, int d, int T, int B) {
    const PackedConv pw = make_pointwise(C);
    const DdsLayerPlan p = plan_dds_layer_lat(C, k, d, false, B, T), ph = plan_dds_layer_lat(C, k, d, true, B, T);
    const std::string sup = fmt("%d %d", dds_layer_lat_supported(pw, C, k, d), dds_lat_grid_ok(B, T));
    if (!p.ok) return sup + " 0 -";
    check_exists(true, p.m == 6 || p.m == 8, "dds_layer_lat_kernel");
    return sup + fmt(" 1 dds_layer_lat_kernel<0, 0, %d> | ", p.m) + grid_fields(p) + fmt(" | <2, 0, %d> lds %zu", ph.m, ph.lds);
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------------------
struct KnobSet {
    const char* name;
    KernelKnobs k;
};
static std::vector<KnobSet> knob_sets() {
    std::vector<KnobSet> v;
    auto add = [&](const char* name, auto set) {
        KernelKnobs k;  // (the defaults of the struct, not of the environment)
        set(k);
        v.push_back({name, k});
    };
    add("default", [](KernelKnobs&) {});
    add("fuse16_maxc=64", [](KernelKnobs& k) { k.fuse16_maxc = 64; });
    add("rb16_narrow_max=0", [](KernelKnobs& k) { k.rb16_narrow_max = 0; });
    add("rbb_c128=0", [](KernelKnobs& k) { k.rbb_c128 = false; });
    add("rbb_c64k11=1", [](KernelKnobs& k) { k.rbb_c64k11 = 1; });
    add("rbb_c64k11=0", [](KernelKnobs& k) { k.rbb_c64k11 = 0; });
    add("rbb_stream_tiles=0", [](KernelKnobs& k) { k.rbb_stream_tiles = 0; });
    add("rbb_stream_tiles=2", [](KernelKnobs& k) { k.rbb_stream_tiles = 2; });
    add("rbb_stream_min_blocks=512", [](KernelKnobs& k) { k.rbb_stream_min_blocks = 512; });
    add("no_rbb_group3", [](KernelKnobs& k) { k.no_rbb_group3 = true; });
    add("no_rbb_group3_c64", [](KernelKnobs& k) { k.no_rbb_group3_c64 = true; });
    add("fuse32_c128=0", [](KernelKnobs& k) { k.fuse32_c128 = false; });
    add("no_convt16s", [](KernelKnobs& k) { k.no_convt16s = true; });
    add("convt16s_all", [](KernelKnobs& k) { k.convt16s_all = true; });
    add("no_convt16l", [](KernelKnobs& k) { k.no_convt16l = true; });
    add("convt16_r128=211", [](KernelKnobs& k) { k.convt16_r128 = 211; });
    add("convt16_r128=311", [](KernelKnobs& k) { k.convt16_r128 = 311; });  // (names no instantiation: the launch is refused)
    add("convt16_split_max=0", [](KernelKnobs& k) { k.convt16_split_max = 0; });
    add("wn16_ncw=2", [](KernelKnobs& k) { k.wn16_ncw = 2; });
    add("flow_ncw=1", [](KernelKnobs& k) { k.flow_ncw = 1; });
    add("flow_narrow_max=0", [](KernelKnobs& k) { k.flow_narrow_max = 0; });
    add("att_valu", [](KernelKnobs& k) { k.att_valu = true; });
    add("att_nw=4", [](KernelKnobs& k) { k.att_nw = 4; });
    add("att_nw=8", [](KernelKnobs& k) { k.att_nw = 8; });
    add("att_short=0", [](KernelKnobs& k) { k.att_short = 0; });
    add("no_att_lat", [](KernelKnobs& k) { k.no_att_lat = true; });
    add("ln_tw=64", [](KernelKnobs& k) { k.ln_tw = 64; });
    add("no_dds_lat", [](KernelKnobs& k) { k.no_dds_lat = true; });
    add("dds_lat_max_blocks=16", [](KernelKnobs& k) { k.dds_lat_max_blocks = 16; });
    return v;
}

struct Grid {
    int T, B;
};
static const Grid kGrid[] = {{1, 1}, {1808, 1}, {8192, 1}, {1808, 4}, {32768, 64}};

int main() {
    std::puts("# P16 C k dil T B : {rbpair16_supported} ok kernel | gx gy gz block lds");
    std::puts("# B16 C k T B : {rbblock16_supported: dilations 1 3 5, dilations 1 3 2, two dilations} ok kernel nt N | gx gy gz block lds");
    std::puts("# G3 C T B : {rbblock16_group3_supported: k = 3 7 11, k = 3 7 7} ok kernel | gx gy gz block lds");
    std::puts("# P32 C k dil T B : {rbpair32_supported} ok kernel | gx gy gz block lds");
    std::puts("# B32 C k T B : {rbblock32_supported: dilations 1 3 5, dilations 1 3 2} ok kernel | gx gy gz block lds");
    std::puts("# CT cin cout stride T B : {convt16_stream_supported: with 16-bit weights, without} ok tag kernel | gx gy gz block lds");
    std::puts("# WN hidden k dil T B : ok32 ok16 kernel | gx gy gz block lds | kernel | gx gy gz block lds   (ok: the shape part of wavenet32_supported / wavenet16_supported)");
    std::puts("# FC hidden half k rate layers T B : ok kernel | gx gy gz block lds | wide N narrow N   (ok: the shape part of flow_couple16_supported)");
    std::puts("# AT heads head_dim window T B : ok kernel | gx gy gz block lds | vshift N (the kernel without matrix cores)");
    std::puts("# LN C T B : ok kernel | gx gy gz block lds     DW C k dil T B : ok | gx gy gz block lds (dds_depthwise_kernel)");
    std::puts("# DL C k dil T B : {dds_layer_supported, fp32} ok kernel | gx gy gz block lds");
    std::puts("# DT C k dil T B : {dds_layer_lat_supported} grid_ok ok kernel | gx gy gz block lds | instantiation and LDS bytes with a 1x1 conv in front");
    std::map<std::string, std::string> base;
    for (const KnobSet& ks : knob_sets()) {
        KernelKnobsScope scope(&ks.k);
        const bool def = base.empty();
        std::printf("## %s\n", ks.name);
        auto emit = [&](const std::string& key, const std::string& fields) {
            std::string& b = base[key];
            if (def) b = fields;
            else if (b == fields) return;
            std::printf("%s : %s\n", key.c_str(), fields.c_str());
        };
        auto pair16 = [&](int C, int k, int d, Grid g) { emit(fmt("P16 %d %d %d %d %d", C, k, d, g.T, g.B), row_rbpair16(C, k, d, g.T, g.B)); };
        auto block16 = [&](int C, int k, Grid g) { emit(fmt("B16 %d %d %d %d", C, k, g.T, g.B), row_rbblock16(C, k, g.T, g.B)); };
        auto group3 = [&](int C, Grid g) { emit(fmt("G3 %d %d %d", C, g.T, g.B), row_group3(C, g.T, g.B)); };
        auto pair32 = [&](int C, int k, int d, Grid g) { emit(fmt("P32 %d %d %d %d %d", C, k, d, g.T, g.B), row_rbpair32(C, k, d, g.T, g.B)); };
        auto block32 = [&](int C, int k, Grid g) { emit(fmt("B32 %d %d %d %d", C, k, g.T, g.B), row_rbblock32(C, k, g.T, g.B)); };
        auto convt = [&](int cin, int cout, int s, Grid g) { emit(fmt("CT %d %d %d %d %d", cin, cout, s, g.T, g.B), row_convt16(cin, cout, s, g.T, g.B)); };
        // every shape on two grids; the shapes with kernels on all of kGrid
        for (int C : {32, 64, 128, 256, 512})
            for (int k : {3, 5, 7, 11}) {
                for (int d : {1, 3, 5, 2})
                    for (const Grid g : kGrid)
                        if (g.T == 1808 || (d == 1 && k != 5 && C <= 256)) pair16(C, k, d, g), pair32(C, k, d, g);
                for (const Grid g : kGrid) block16(C, k, g), block32(C, k, g);
            }
        for (int C : {32, 64, 128})
            for (const Grid g : kGrid) group3(C, g);
        // rb16_narrow_max: 128 and 129 blocks of four 32-column tiles, as one utterance and as eight
        for (int C : {128, 256})
            for (int k : {3, 7, 11}) {
                const int bo4 = rbpair16_geom(k, 1, C, 4).bo;
                for (const Grid g : {Grid{128 * bo4, 1}, Grid{128 * bo4 + 1, 1}, Grid{16 * bo4, 8}, Grid{16 * bo4 + 1, 8}}) pair16(C, k, 3, g);
            }
        // rbblock16's segments: one-tile block counts around two rounds of VITS_RBB_STREAM_MIN_BLOCKS and around every further tile up to each shape's cap
        for (int C : {32, 64, 128})
            for (int k : {3, 7, 11}) {
                if (!rbblock16_exists(k, C)) continue;
                const int bo = rbblock16_geom(k, C).bo;
                for (int n : {3071, 3072, 4607, 4608, 6143, 6144, 9215, 9216}) block16(C, k, {bo * n, 1});
                for (int n : {47, 48, 96, 144}) block16(C, k, {bo * n, 64});
            }
        // the grouped launch's 3072 blocks
        for (int C : {32, 64}) {
            const int bo = rbblock16_geom(7, 64).bo;
            for (const Grid g : {Grid{3072 * bo, 1}, Grid{3072 * bo + 1, 1}, Grid{1024 * bo, 3}, Grid{1024 * bo + 1, 3}, Grid{48 * bo, 64}, Grid{48 * bo + 1, 64}}) group3(C, g);
        }
        // transposed convs: the upsamplers of the two synthetic architectures, c_in = 512, rows <= 128 and > 128, strides that are no multiple of 4, every instantiation
        struct Up {
            int cin, cout, s;
        };
        for (const Up u : {Up{512, 256, 8}, Up{256, 128, 8}, Up{128, 64, 2}, Up{64, 32, 2}, Up{32, 16, 4}, Up{16, 8, 2}, Up{512, 64, 2}, Up{320, 64, 2}, Up{64, 64, 2}, Up{128, 32, 2},
                           Up{192, 32, 2}, Up{256, 128, 2}, Up{256, 64, 3}, Up{128, 64, 4}, Up{576, 64, 2}, Up{128, 48, 2}}) {
            for (const Grid g : kGrid) convt(u.cin, u.cout, u.s, {g.T / 8 + 1, g.B});
            // convt16_split_max: 64 and 65 tiles of 128 and of 64 positions
            for (int bn : {64, 128})
                if (u.cout * u.s > 128)  // (only the four-phase kernel deals a tile out over several blocks)
                    for (const Grid g : {Grid{64 * bn - 1, 1}, Grid{64 * bn, 1}, Grid{8 * bn - 1, 8}, Grid{8 * bn, 8}}) convt(u.cin, u.cout, u.s, g);
        }
        // the flow: one WaveNet layer, one coupling layer; 96 and 97 blocks of 48 frames
        const int bo48 = flow_couple16_geom(2, 2).bo;
        std::vector<Grid> fg(kGrid, kGrid + sizeof(kGrid) / sizeof(Grid));
        for (Grid& g : fg) g.T = g.T / 8 + 1;
        for (const Grid g : {Grid{96 * bo48, 1}, Grid{96 * bo48 + 1, 1}, Grid{24 * bo48, 4}, Grid{24 * bo48 + 1, 4}}) fg.push_back(g);
        struct Flow {
            int hidden, half, k, rate, layers;
        };
        for (const Flow f : {Flow{192, 96, 5, 1, 4}, Flow{128, 64, 5, 1, 4}, Flow{192, 96, 3, 1, 4}, Flow{192, 96, 5, 2, 4}, Flow{192, 96, 5, 1, 3}, Flow{192, 48, 5, 1, 4}})
            for (const Grid g : fg) {
                emit(fmt("FC %d %d %d %d %d %d %d", f.hidden, f.half, f.k, f.rate, f.layers, g.T, g.B), row_flow(f.hidden, f.half, f.k, f.rate, f.layers, g.T, g.B));
                if (f.layers == 4 && f.half == 96) emit(fmt("WN %d %d %d %d %d", f.hidden, f.k, f.rate, g.T, g.B), row_wavenet(f.hidden, f.k, f.rate, g.T, g.B));
            }
        // attention: every head size on short and long sequences; the lengths at which one block's scores pass half the CU's LDS (four -> eight waves) and all
        // of it (-> the kernel without matrix cores); 512 / 513 tokens (short variant); 128 / 129 blocks (latency variant) and 512 / 513 (VALU block size); windows
        auto att = [&](int heads, int hd, int w, Grid g) { emit(fmt("AT %d %d %d %d %d", heads, hd, w, g.T, g.B), row_attention(heads, hd, w, g.T, g.B)); };
        for (int hd : {16, 24, 64, 96, 112, 128, 144}) {
            int t_half = 1, t_full = 1;
            while (2 * att_mfma_lds(hd, t_half, 4) <= kLdsMax) ++t_half;
            while (att_mfma_lds(hd, t_full, 4) <= kLdsMax) ++t_full;
            for (int T : {12, 512, 513, t_half - 1, t_half, t_full - 1, t_full, 2400})
                for (int B : {1, 8})
                    if (B == 1 || T == 512 || T == 513) att(2, hd, 4, {T, B});
            for (const Grid g : {Grid{2048, 1}, Grid{2049, 1}}) att(1, hd, 4, g);                            // 128 / 129 blocks
            for (const Grid g : {Grid{256, 4}, Grid{257, 4}, Grid{256, 16}, Grid{257, 16}}) att(2, hd, 4, g);  // 128 / 136 and 512 / 544 blocks
            for (int w : {0, 33})
                for (int T : {128, 1100}) att(2, hd, w, {T, 2});
        }
        // LayerNorm: channel counts on both sides of 64 KB and of 150 KB of LDS, for the 32-step tile and (VITS_LN_TW=64) the 64-step tile
        for (int C : {192, 224, 225, 480, 481, 512, 568, 569, 1168, 1169})
            for (const Grid g : {Grid{8, 1}, Grid{150, 2}, Grid{1025, 64}}) emit(fmt("LN %d %d %d", C, g.T, g.B), row_layer_norm(C, g.T, g.B));
        // DDS: 2, 3, 5, 6, 7, 8 chunks of 32 channels and what the kernels refuse; dilations 1, 3, 9; 96 and 97 blocks of 16 tokens
        for (int C : {48, 64, 96, 160, 192, 224, 256, 288, 512})
            for (int k : {3, 2})
                for (int d : {1, 9})
                    for (const Grid g : {Grid{128, 1}, Grid{1536, 1}, Grid{1537, 1}, Grid{256, 6}, Grid{257, 6}}) {
                        if ((k == 2 && d != 1) || ((C == 48 || C >= 288 || k == 2) && g.B != 1)) continue;
                        emit(fmt("DL %d %d %d %d %d", C, k, d, g.T, g.B), row_dds_layer(C, k, d, g.T, g.B));
                        emit(fmt("DT %d %d %d %d %d", C, k, d, g.T, g.B), row_dds_lat(C, k, d, g.T, g.B));
                        if (g.T <= 256 && C >= 192) emit(fmt("DW %d %d %d %d %d", C, k, d, g.T, g.B), row_depthwise(C, k, d, g.T, g.B));
                    }
    }
    return g_missing ? 1 : 0;
}
