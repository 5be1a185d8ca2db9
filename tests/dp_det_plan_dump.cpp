// dp_det_plan_dump — prints the launch policy of the deterministic duration predictor's fused kernel (plan_dp_det, vits.cpp_amd/csrc/launch_plan.cpp) over a
// fixed sweep of shapes, grids, variants and knob sets, one line per case: tests/test_detdp_host.py compares the output with tests/golden/dp_det_plan_table.txt
// byte for byte. Links launch_plan.o alone (csrc/Makefile, target dp_det_plan_dump): the policy touches no device.
//
// Lines: `DP hidden filter k variant T B : <fields>`; fields = `fused kernel | gx gy gz block lds` for a launch of dp_det_kernel, `unfused` where the engine runs the
// un-fused sequence, `refused` where a forced tile (variant 1 / 2) has no instantiation. The default knob set prints every case, every other one the cases whose
// line differs. Exits non-zero if a launchable plan names an instantiation dp_det_exists denies, or one whose LDS is not the geometry function's.
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>

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
static int g_missing = 0;

static std::string row(int H, int FC, int k, int variant, int T, int B) {
    const DpDetPlan p = plan_dp_det(H, FC, k, B, T, variant);
    if (!p.ok) return (variant == 1 || variant == 2) ? "refused" : "unfused";
    const int hch = blocks_for(H, 32);
    const std::string kernel = fmt("dp_det_kernel<%d, %d, %d, %d>", hch, FC, k, p.nt);
    const DpDetGeom g = dp_det_geom(hch, FC, k, p.nt);
    if (!p.fused || !dp_det_exists(H, FC, k, p.nt) || g.lds != p.lds || g.block != p.block || g.lds > kLdsMax || p.gx != blocks_for(T, p.nt) || p.gy != B) {
        std::fprintf(stderr, "no such instantiation, or a plan that is not its geometry: %s\n", kernel.c_str());
        ++g_missing;
    }
    return "fused " + kernel + " | " + fmt("%d %d %d %d %zu", p.gx, p.gy, p.gz, p.block, p.lds);
}

struct KnobSet {
    const char* name;
    KernelKnobs k;
};

int main() {
    std::puts("# DP hidden filter k variant T B : fused kernel | gx gy gz block lds   or   unfused   or   refused (variant: 0 planner, 1 16-token tile, 2 wide tile, 3 un-fused)");
    KnobSet sets[4];
    sets[0].name = "default";
    sets[1].name = "no_dp_det_fuse", sets[1].k.no_dp_det_fuse = true;
    sets[2].name = "dp_det_lat_max_blocks=8", sets[2].k.dp_det_lat_max_blocks = 8;
    sets[3].name = "dp_det_lat_max_blocks=0", sets[3].k.dp_det_lat_max_blocks = 0;
    struct Shape {
        int H, FC, k;
    };
    struct Grid {
        int T, B;
    };
    std::map<std::string, std::string> base;
    for (const KnobSet& ks : sets) {
        KernelKnobsScope scope(&ks.k);
        const bool def = base.empty();
        std::printf("## %s\n", ks.name);
        // the three shapes with instantiations, then what the fused kernel refuses: another hidden size, another filter size, an even / a seven-tap kernel
        for (const Shape s : {Shape{192, 256, 3}, Shape{192, 256, 5}, Shape{16, 32, 3}, Shape{128, 256, 3}, Shape{192, 192, 3}, Shape{192, 256, 7}, Shape{16, 32, 5}, Shape{192, 256, 2}})
            for (int variant : {0, 1, 2, 3})
                // one token; batch 1 x 128 ids; 96 and 97 blocks of 16 tokens as one utterance and as six; 8 and 9 blocks; the benchmark batch
                for (const Grid g : {Grid{1, 1}, Grid{128, 1}, Grid{129, 1}, Grid{1536, 1}, Grid{1537, 1}, Grid{256, 6}, Grid{257, 6}, Grid{128, 64}}) {
                    const std::string key = fmt("DP %d %d %d %d %d %d", s.H, s.FC, s.k, variant, g.T, g.B), fields = row(s.H, s.FC, s.k, variant, g.T, g.B);
                    std::string& b = base[key];
                    if (def) b = fields;
                    else if (b == fields) continue;
                    std::printf("%s : %s\n", key.c_str(), fields.c_str());
                }
    }
    return g_missing ? 1 : 0;
}
