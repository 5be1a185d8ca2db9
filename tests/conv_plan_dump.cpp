// conv_plan_dump — prints the convolutions' launch policy (vits.cpp_amd/csrc/conv_plan.cpp) over a fixed sweep of layers, lengths, batches and knob
// sets as text, one line per case: tests/test_conv_plan_host.py compares the output with tests/golden/conv_plan_table.txt byte for byte.
// Links conv_plan.o alone (csrc/Makefile, target conv_plan_dump): the policy touches no device.
//
// Lines (fields separated by one blank; the header lines starting with '#' name them):
//   F  one fp32 launch (plan_conv)          G  one 16-bit launch (plan_conv16)      L  one grouped conv16_lat launch      P  the vocoder's conv_pre
// A line '@' names the layer of the lines behind it. The default knob set prints every case; every other knob set prints the cases whose line differs from the
// default one, on a thinner grid; "planes 0" lines (no latency-kernel copy of the weights) likewise only where they differ from "planes 1".
// Every layer is walked over a part of the (length, batch) grid that rotates with the layer's position in the list, so that the table stays small.
// Exits non-zero if a plan marked launchable names an instantiation that the launchers' own predicates (conv_tile_exists and its kin) say does not exist.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/conv_plan.h"

using namespace vits;

struct Layer {
    int epi, k, cin, cout, stride, dil;
};
struct Grid {
    int T, B;
};
// every length at batch 1, every batch at 128 and 129 ids' worth of columns, the long end at large batches
static const Grid kGrid[] = {{1, 1},   {16, 1},  {17, 1},  {32, 1},   {33, 1},   {128, 1},  {129, 1},  {256, 1},   {257, 1},  {1024, 1}, {8192, 1},
                             {128, 2}, {128, 4}, {129, 8}, {128, 64}, {257, 4}, {1024, 8}, {1024, 64}, {8192, 64}};
static const size_t kRotate = 7;  // a layer takes every kRotate-th pair of its grid (and always 128 x 1)
static bool in_knob_grid(Grid g) {  // the knob sets other than the default walk these pairs of kGrid only
    for (Grid k : {Grid{33, 1}, Grid{128, 1}, Grid{1024, 1}, Grid{128, 4}, Grid{129, 8}, Grid{128, 64}, Grid{1024, 64}, Grid{8192, 64}})
        if (k.T == g.T && k.B == g.B) return true;
    return false;
}

static std::vector<Layer> layers() {
    std::vector<Layer> v;
    auto add = [&](int epi, int k, int cin, int cout, int stride = 0, int dil = 1) { v.push_back({epi, k, cin, cout, stride, dil}); };
    // SYNTH_FULL (MMS-TTS): encoder, duration predictor, flow, posterior encoder, vocoder
    for (int co : {576, 192, 384, 29}) add(EPI_STD, 1, 192, co);
    add(EPI_STD, 1, 96, 192), add(EPI_STD, 1, 192, 96), add(EPI_STD, 1, 513, 192);
    add(EPI_STD, 3, 192, 768), add(EPI_STD, 3, 768, 192), add(EPI_GATE, 5, 192, 384), add(EPI_STD, 7, 192, 512);
    add(EPI_CONVT, 16, 512, 256, 8), add(EPI_CONVT, 16, 256, 128, 8), add(EPI_CONVT, 4, 128, 64, 2), add(EPI_CONVT, 4, 64, 32, 2);
    // SYNTH_TINY
    for (int co : {48, 16, 32, 29, 8}) add(EPI_STD, 1, 16, co);
    add(EPI_STD, 1, 8, 16), add(EPI_STD, 1, 9, 16);
    add(EPI_STD, 3, 16, 32), add(EPI_STD, 3, 32, 16), add(EPI_GATE, 5, 16, 32), add(EPI_STD, 7, 16, 32);
    add(EPI_CONVT, 8, 32, 16, 4), add(EPI_CONVT, 4, 16, 8, 2);
    for (int c : {16, 8}) {
        for (int d : {1, 3}) add(EPI_STD, 3, c, c, 0, d);
        for (int d : {1, 2}) add(EPI_STD, 5, c, c, 0, d);
    }
    // ResBlock convs
    for (int c : {32, 64, 128, 256, 512})
        for (int k : {3, 7, 11})
            for (int d : {1, 3, 5}) add(EPI_STD, k, c, c, 0, d);
    // run-time dilations, a standard k = 5, the gated conv at dilation 2, degenerate channel counts
    for (int d : {2, 4}) add(EPI_STD, 3, 128, 128, 0, d), add(EPI_STD, 7, 256, 256, 0, d), add(EPI_STD, 11, 64, 64, 0, d);
    add(EPI_STD, 5, 192, 192), add(EPI_GATE, 5, 192, 384, 0, 2);
    add(EPI_STD, 3, 1, 192), add(EPI_STD, 1, 80, 192), add(EPI_STD, 7, 80, 512), add(EPI_STD, 7, 32, 1), add(EPI_STD, 1, 192, 1);
    return v;
}

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
    add("narrow_tiles=0", [](KernelKnobs& k) { k.narrow_tiles = 0; });
    add("tile128=0", [](KernelKnobs& k) { k.tile128 = 0; });
    add("min_blocks=1", [](KernelKnobs& k) { k.min_blocks = 1; });
    add("nbuf=3", [](KernelKnobs& k) { k.nbuf = 3; });
    add("no_oneshot", [](KernelKnobs& k) { k.no_oneshot = true; });
    add("no_narrow", [](KernelKnobs& k) { k.no_narrow = true; });
    add("narrow_k1=0", [](KernelKnobs& k) { k.narrow_k1 = 0; });
    add("no_lat16", [](KernelKnobs& k) { k.no_lat16 = true; });
    add("lat16_max_waves=0", [](KernelKnobs& k) { k.lat16_max_waves = 0; });
    add("db_min=2", [](KernelKnobs& k) { k.db_min = 2; });
    add("t16_tile0=1", [](KernelKnobs& k) { k.t16_tile0 = 1; });
    add("t16_tile0=2", [](KernelKnobs& k) { k.t16_tile0 = 2; });
    add("t16_tile0=3", [](KernelKnobs& k) { k.t16_tile0 = 3; });
    add("t16_tile0=4", [](KernelKnobs& k) { k.t16_tile0 = 4; });
    add("no_lat16h", [](KernelKnobs& k) { k.no_lat16h = true; });
    add("lat16h_max_tiles_c128=4096", [](KernelKnobs& k) { k.lat16h_max_tiles_c128 = 4096; });
    add("lat16h_shape=22", [](KernelKnobs& k) { k.lat16h_shape = 22; });
    add("lat16h_shape=42", [](KernelKnobs& k) { k.lat16h_shape = 42; });
    add("lat16h_group_shape=41", [](KernelKnobs& k) { k.lat16h_group_shape = 41; });
    add("lat16h_group_shape=22", [](KernelKnobs& k) { k.lat16h_group_shape = 22; });
    add("lat16h_group_shape=42", [](KernelKnobs& k) { k.lat16h_group_shape = 42; });
    return v;
}

static float g_dummy[8];  // (pointers are only tested for null)
static uint16_t g_dummy16[8];

// planes: 1 = with the latency kernel's weight copy (where the layer is a candidate), the 16-bit planes and the split planes (candidates); 0 = fp32 weights only
static PackedConv make_conv(const Layer& l, bool planes) {
    PackedConv w;
    const ConvPackDims d = conv_pack_dims(l.cout, l.cin, l.k, l.epi, l.stride);
    w.cin = l.cin, w.cout = l.cout, w.kt = d.kt, w.rows = d.rows, w.mtiles = d.mtiles, w.mtiles_used = d.mtiles_used, w.nchunks = d.nchunks;
    w.epi = l.epi, w.ct_stride = l.stride;
    w.wp = g_dummy, w.bias = g_dummy;
    if (planes && conv_lat16_candidate(l.epi, d.kt, l.cin)) w.wp_l16 = g_dummy;
    if (planes) w.wp16 = g_dummy16;
    if (planes && conv_split_candidate(l.epi, d.kt, l.cin, l.cout)) w.wps = g_dummy16;
    return w;
}

static std::string key(char kind, int planes, Grid g) {
    char b[64];
    std::snprintf(b, sizeof(b), "%c %d %d %d", kind, planes, g.T, g.B);
    return b;
}

// A plan the planner calls launchable names an instantiation that exists, by the launchers' own predicates (not by the plan's `ok`, which folds them in)
static int g_missing = 0;
static void check_exists(bool ok, bool exists, const char* who, const Layer& l, Grid g) {
    if (!ok || exists) return;
    std::fprintf(stderr, "%s: no such instantiation for epi %d k %d cin %d cout %d dil %d, T %d B %d\n", who, l.epi, l.k, l.cin, l.cout, l.dil, g.T, g.B);
    ++g_missing;
}

static std::string fp32_case(const Layer& l, bool planes, Grid g) {
    const PackedConv w = make_conv(l, planes);
    ConvCall c;
    c.x.p = c.y.p = g_dummy;
    c.batch = g.B, c.t_in = g.T, c.t_out = l.epi == EPI_CONVT ? g.T * l.stride : g.T;
    c.dil = l.dil, c.pad_l = l.epi == EPI_CONVT ? 0 : (w.kt - 1) * l.dil / 2;
    const ConvPlan p = plan_conv(w, c);
    check_exists(p.ok, p.tile == TILE_LAT16 ? conv_lat16_exists(w.epi, p.pitch) : p.dil_ct != kNoKernel && conv_tile_exists(w.epi, w.kt, p.dil_ct, p.db, p.tile), "plan_conv", l, g);
    char b[256];
    std::snprintf(b, sizeof(b), " : %d %d %d %d %d %d %d %d %d %zu %d %d %d %d %d %d %d%d%d%d", p.ok, p.tile, p.dil, p.dil_ct, p.db, p.gx, p.gy, p.gz, p.block, p.lds, p.xw, p.lds_off,
                  p.nbuf, p.oneshot, p.pitch, p.ln_ok, conv_group_supported(w, l.dil), conv_split_supported(w, l.dil), conv_split_candidate(w.epi, w.kt, w.cin, w.cout),
                  conv_lat16_candidate(w.epi, w.kt, w.cin));
    return b;
}

static Conv16Call call16(const Layer& l, const PackedConv& w, bool group, Grid g) {
    Conv16Call c;
    c.x.p = g_dummy16;
    c.batch = g.B, c.t_in = g.T, c.t_out = l.epi == EPI_CONVT ? g.T * l.stride : g.T;
    c.dil = l.dil, c.pad_l = l.epi == EPI_CONVT ? 0 : (w.kt - 1) * l.dil / 2;
    if (group) c.yg = g_dummy, c.y16.p = g_dummy16;
    else c.y.p = g_dummy;
    return c;
}
static std::string lat_fields(const Conv16LatPlan& l) {
    char b[128];
    std::snprintf(b, sizeof(b), "%d %d %d %d %d %d %d %zu", l.wm, l.nr, l.pitch, l.gx, l.gy, l.gz, l.block, l.lds);
    return b;
}
static std::string conv16_case(const Layer& l, bool group, Grid g) {
    const PackedConv w = make_conv(l, true);
    const Conv16Call c = call16(l, w, group, g);
    const Conv16Plan p = plan_conv16(w, c);
    check_exists(p.ok, p.lat ? conv16_lat_shape_exists(10 * p.l.wm + p.l.nr, false) : p.dil_ct != kNoKernel && conv16_tile_exists(p.epi16, p.dil_ct, p.tile), "plan_conv16", l, g);
    char b[256];
    std::snprintf(b, sizeof(b), " : %d %d %d %d %d %d %d %d %d %d %d %zu %d %d %d %d%d | ", p.ok, p.lat, p.epi16, p.chosen, p.tile, p.part, p.dil, p.dil_ct, p.gx, p.gy, p.gz, p.lds, p.xwp,
                  p.lds_off, p.nbuf, conv16_lat_shape_ok(w.cin, w.kt, l.dil, g.B, c.t_out), conv16_lat_wanted(w, c));
    return b + lat_fields(p.l);
}
// the same-position convs (k = 3, 7, 11) of a C-channel stage's resblocks as one conv16_lat launch
static std::string lat_group_case(int C, int dil, Grid g) {
    PackedConv w[3];
    Conv16Call c[3];
    const PackedConv* wp[3];
    const int kts[3] = {3, 7, 11};
    for (int i = 0; i < 3; ++i) {
        const Layer l = {EPI_STD, kts[i], C, C, 0, dil};
        w[i] = make_conv(l, true), c[i] = call16(l, w[i], true, g), wp[i] = &w[i];
    }
    const bool wanted = conv16_lat_group_wanted(wp, c);
    return " : " + std::to_string(wanted) + " | " + (wanted ? lat_fields(plan_conv16_lat(C, C, 11, dil, kernel_knobs().lat16h_group_shape, g.T, 3 * g.B)) : std::string("-"));
}
static std::string lat_pre_case(const Layer& l, Grid g) {
    const PackedConv w = make_conv(l, true);
    const bool wanted = conv16_lat_pre_wanted(w, g.B, g.T);
    return " : " + std::to_string(wanted) + " | " + (wanted ? lat_fields(plan_conv16_lat(l.cin, l.cout, w.kt, 1, 21, g.T, g.B)) : std::string("-"));
}

int main() {
    std::vector<Layer> L = layers();
    for (int C : {128, 256})
        for (int d : {1, 3, 5}) L.push_back({EPI_STD, 0, C, C, 0, d});  // (k = 0: the grouped conv16_lat launch of a stage's k = 3, 7, 11 convs)
    // a standard conv with 2 taps: no tile kernel has them; conv_lat16_kernel (taps at run time) runs it on tiny grids, every other launch is refused
    L.push_back({EPI_STD, 2, 32, 384, 0, 1}), L.push_back({EPI_STD, 2, 192, 192, 0, 1});
    std::puts("# @ epi k cin cout stride dil");
    std::puts("# F planes T B : ok tile dil dil_ct db gx gy gz block lds xw lds_off nbuf oneshot pitch ln_ok {group_supported split_supported split_candidate lat16_candidate}");
    std::puts("# G group_layout T B : ok lat epi16 chosen tile part dil dil_ct gx gy gz lds xwp lds_off nbuf {lat_shape_ok lat_wanted} | wm nr pitch gx gy gz block lds");
    std::puts("# L 1 T B : group_wanted | wm nr pitch gx gy gz block lds     P 1 T B : pre_wanted | wm nr pitch gx gy gz block lds");
    std::map<std::string, std::string> base;
    for (const KnobSet& ks : knob_sets()) {
        KernelKnobsScope scope(&ks.k);
        const bool def = base.empty();
        std::printf("## %s\n", ks.name);
        for (size_t li = 0; li < L.size(); ++li) {
            const Layer& l = L[li];
            bool named = false;
            auto emit = [&](const std::string& k, const std::string& fields, const std::string* same_as = nullptr) {
                std::string& b = base[std::to_string(li) + k];
                if (def) b = fields;
                if (def ? same_as && *same_as == fields : b == fields) return;
                if (!named) std::printf("@ %d %d %d %d %d %d\n", l.epi, l.k, l.cin, l.cout, l.stride, l.dil);
                named = true;
                std::printf("%s%s\n", k.c_str(), fields.c_str());
            };
            for (size_t i = 0; i < sizeof(kGrid) / sizeof(Grid); ++i) {
                const Grid g = kGrid[i];
                if ((i + li) % kRotate && !(g.T == 128 && g.B == 1)) continue;
                if (!def && !in_knob_grid(g)) continue;
                if (!l.k) {
                    emit(key('L', 1, g), lat_group_case(l.cin, l.dil, g));
                    continue;
                }
                const std::string with = fp32_case(l, true, g);
                emit(key('F', 1, g), with);
                emit(key('F', 0, g), fp32_case(l, false, g), &with);
                if (l.epi == EPI_STD && l.k == 2) continue;  // (the 16-bit dispatchers have no standard conv with 2 taps at all: nothing to pin)
                emit(key('G', 0, g), conv16_case(l, false, g));
                if (l.epi != EPI_GATE && (l.cout & 7) == 0) emit(key('G', 1, g), conv16_case(l, true, g));
                if (l.epi == EPI_STD && l.k == 7 && l.cin != l.cout) emit(key('P', 1, g), lat_pre_case(l, g));
            }
        }
    }
    return g_missing ? 1 : 0;
}
