// vocoder_plan.h — how the resblocks of a HiFi-GAN stage are scheduled, as plain host arithmetic beside conv_plan.h and launch_plan.h: which kernel each
// resblock runs on, and whether the stage's resblocks chain through the shared sum, run side by side or go out as grouped launches. No kernels, no HIP calls:
// run_vocoder_window16 / run_vocoder_window32 (engine_vocoder.cpp) build the call structs and launch what the plan says, Engine::plan_tile_maps plans lists for
// the widths of the kernels the plan names, and vits_op_resblock's variant 0 asks the same per-resblock rule. tests/vocoder_plan_dump.cpp links vocoder_plan.o,
// conv_plan.o and launch_plan.o alone and freezes the schedule as a table. The orchestrator's knobs arrive in VocPolicy; the launch functions' own (KernelKnobs)
// come from kernel_knobs(), as in the other planners.
#pragma once
#include "../../include/vits.h"
#include "conv_plan.h"
#include "launch_plan.h"

namespace vits {

// plain views of a stage's weights
struct ResBlockW {
    std::vector<PackedConv> c1, c2;
    std::vector<int> dil;
    int k;
    // the three conv pairs as the whole-resblock kernels take them
    void pairs3(const PackedConv* (&w1)[3], const PackedConv* (&w2)[3]) const {
        for (int d = 0; d < 3; ++d) w1[d] = &c1[d], w2[d] = &c2[d];
    }
};
struct UpStageW {
    PackedConv up;
    std::vector<ResBlockW> rbs;
    int channels, stride, k;
};

// What the decisions read of the handle and of the call, filled once per call (Engine::voc_policy). The defaults are the handle's: Engine::Knobs.
struct VocPolicy {
    int rb_streams = 3, rb16_serial_max_frames = 1300, rb16_serial_min_frames = 600, rb32_sum3_max_frames = 2000, lrelu_copy_minc = 128;
    bool no_rbblock16 = false, no_fuse32 = false, no_rbblock32 = false, no_rb_group = false, rb_group_always = false;
    bool prof_on = false;            // the per-kernel profiler: its events need kernels that do not overlap
    bool fuse16 = true;              // Call::fuse16: the 16-bit group layout with fused kernels
    int arith_now = VITS_ARITH_F32;  // what the dispatchers see (VITS_ARITH_F32 under the split arithmetic too)
    bool split_on = false;           // VITS_ARITH_F32_SPLIT ...
    bool split_planes = false;       // ... and the call has the buffers of the split planes
    bool aligned = true;             // the fp32 fused kernels' 16-byte loads: every stage buffer 16-byte aligned, every stride a multiple of four floats
};

// The kernel of one resblock. Convs: two launches per conv pair; Split: the same on the split-operand kernels (conv_split.hip); Pairs: one fused kernel per pair
// (rbpair16.hip / rbpair32.hip; all pairs of a resblock or none); Block: the whole resblock as one kernel (rbblock16.hip / rbblock32.hip)
enum class RbKernel : int { Convs = 0, Split = 1, Pairs = 2, Block = 3 };
// what every conv of a resblock carries (the fused kernels have no form without a bias; each kernel family reads its own weight planes); split: every conv
// passes conv_split_supported
struct RbHas {
    bool bias = true, wp = true, wp16 = true, split = false;
};
RbHas rb_has(const ResBlockW& R);
// The per-resblock rule, once per layout. 16-bit: the whole-resblock kernel, else fused pairs unless every pair goes to conv16_lat_kernel, else two launches per pair
RbKernel rb_kernel16(int C, int k, const int* dil, int nd, RbHas has, int B, int t_out, const VocPolicy& p);
// fp32: a resblock the split kernels take runs on them; otherwise the whole-resblock kernel, else fused pairs, else two launches per pair
RbKernel rb_kernel32(int C, int k, const int* dil, int nd, RbHas has, const VocPolicy& p);

// The side streams and the per-chain buffers know three resblocks per stage: a plan names the kernels of the first three. A stage with more runs them one
// behind the other on one stream, the further ones without a whole-resblock kernel (16-bit: rb_kernel16_of) / as two launches per pair (fp32: kernel_of).
constexpr int kVocRb = 3;
struct VocStage16Plan {
    RbKernel rb[kVocRb] = {RbKernel::Convs, RbKernel::Convs, RbKernel::Convs};
    bool all_block = false;      // every resblock a whole-resblock kernel: nobody reads the 16-bit copy of the stage input
    bool par = false;            // one stream per resblock
    bool sum3 = false;           // side by side: own outputs + one sum launch
    bool longest_first = false;  // ... enqueued last resblock first
    bool group3 = false;         // side-by-side whole-resblock kernels as ONE launch (rbblock16_group3_kernel) + the sum, on the main stream
    bool lat3 = false;           // side-by-side latency convs: the same-position convs of the three resblocks as one launch each (conv16_lat_group_kernel) + the sum
    bool block(size_t j) const { return j < (size_t)kVocRb && rb[j] == RbKernel::Block; }
};
struct VocStage32Plan {
    RbKernel rb[kVocRb] = {RbKernel::Convs, RbKernel::Convs, RbKernel::Convs};
    bool any_split = false;  // the stage input is also written as split planes
    bool grouped = false;    // the same-position convs of the un-fused resblocks as one launch each (conv_group_kernel)
    bool par = false, sum3 = false;
    bool lcopy = false;      // the stream is also stored activated, for the first conv of each pair
    RbKernel kernel_of(size_t j) const { return j < (size_t)kVocRb ? rb[j] : RbKernel::Convs; }
    bool fused(size_t j) const { return kernel_of(j) >= RbKernel::Pairs; }
};
// frames: the frames of the window over all utterances (WinCtx::ssum[0]); t_out: the longest utterance behind the stage's upsampler
VocStage16Plan plan_voc_stage16(const UpStageW& U, int B, int t_out, int64_t frames, const VocPolicy& p);
VocStage32Plan plan_voc_stage32(const UpStageW& U, int B, int t_out, int64_t frames, const VocPolicy& p);
RbKernel rb_kernel16_of(const VocStage16Plan& pl, const UpStageW& U, size_t j, int B, int t_out, const VocPolicy& p);  // resblock j of the stage `pl` was planned for
// 16-bit: conv_pre reads the fp32 flow output itself, on conv16_lat_kernel (no converter launch). F: the flow's channels, Lw: the window's longest utterance
bool plan_voc_pre_lat(const PackedConv& pre, int F, int B, int Lw, const VocPolicy& p);

}  // namespace vits
