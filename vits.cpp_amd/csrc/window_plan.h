// window_plan.h — the vocoder windows of one call (long-form / streaming, vits.h vocoder_chunk_frames), stated once for every reader: the window loop and the
// streaming sink (engine.cpp), the lists of existing tiles (Engine::plan_tile_maps), the streaming range tables (Engine::upload_ranges) and the arena layout
// (engine_flow.cpp). Window w owns frames [f0, f1) and computes frames [lo, hi) = the owned range widened by the vocoder's receptive field: every sample it
// emits sees exactly the inputs it sees in a whole-utterance run, in the same order of accumulation, so the PCM is bit-identical while the activations are
// bounded by the window. Plain host arithmetic: no kernels, no HIP calls, no Engine; tests/window_plan_dump.cpp links window_plan.o alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace vits {

struct WindowPlan {
    struct Win {
        int f0, f1, lo, hi;
    };
    // The plan reads the caller's arrays, which outlive it (Call::frames / smul / sadd): frames [B], every one >= 1; smul / sadd [n_up + 1], the length of
    // vocoder stage i as the affine function L * smul[i] + sadd[i] of a frame count. A call that is not windowed allocates its one window and nothing else.
    const int* frames = nullptr;
    const int *smul = nullptr, *sadd = nullptr;
    int B = 0, n_up = 0;
    int Lmax = 0;   // the longest utterance's frames
    int M = 1;      // samples per frame (smul[n_up])
    int Lw_max = 0; // the widest window's computed frames
    bool windowed = false;
    std::vector<Win> wins;

    // chunk: the frames a window owns, as the call asked (vocoder_chunk_frames). No chunking asked for, a chunk at least as long as the longest utterance
    // (which the caller cannot know in advance) or collect_taps give ONE window: a streaming sink then gets each utterance in a single call.
    void plan(const int* frames, int B, const int* smul, const int* sadd, int n_up, int halo_frames, int chunk, bool collect_taps);

    size_t size() const { return wins.size(); }
    const Win& operator[](size_t w) const { return wins[w]; }

    // ---- lengths inside a window (window-local: what the device holds in d_len[i] of window w) ----
    // frames of utterance b that window w computes; <= 0: the utterance has nothing in the window
    int frames_in(size_t w, int b) const { return std::min(frames[b], wins[w].hi) - wins[w].lo; }
    int stage_of(int lf, int i) const { return lf <= 0 ? 0 : lf * smul[i] + sadd[i]; }
    int len(size_t w, int i, int b) const { return stage_of(frames_in(w, b), i); }
    // the longest an utterance can be at stage i of window w, and (profiler accounting, the vocoder planner) the sum over the utterances
    int stage_max(size_t w, int i) const { return (wins[w].hi - wins[w].lo) * smul[i] + sadd[i]; }
    int64_t stage_sum(size_t w, int i) const;

    // ---- emitted samples ----
    // Of the samples a window computes, [emit_lo, emit_end) (window-local; window-local sample 0 is global sample lo * M) are the utterance's own. The window
    // holding the utterance's end also emits its no-crop tail sadd[n_up] (Q1); the same columns of longer utterances are not final yet.
    bool owns(size_t w, int b) const { return frames[b] > wins[w].f0; }        // the utterance has frames the window owns
    bool ends_in(size_t w, int b) const { return frames[b] <= wins[w].f1; }    // ... and its last one is among them (given owns)
    int emit_lo(size_t w) const { return (wins[w].f0 - wins[w].lo) * M; }
    int emit_end(size_t w, int b) const {
        if (!owns(w, b)) return 0;
        return ends_in(w, b) ? (frames[b] - wins[w].lo) * M + sadd[n_up] : (wins[w].f1 - wins[w].lo) * M;
    }
    // After window w the model-rate samples [0, E_w) of an utterance are final: everything once it has ended, else up to the end of the frames the window
    // owns (given owns; a window that owns nothing of an utterance leaves E where it was).
    int64_t final_end(size_t w, int b) const { return ends_in(w, b) ? (int64_t)frames[b] * M + sadd[n_up] : (int64_t)wins[w].f1 * M; }
    // the plain streaming chunk of an utterance the window owns frames of: global samples [chunk_begin, final_end)
    int64_t chunk_begin(size_t w) const { return (int64_t)wins[w].f0 * M; }
    // the columns of the rows (at `stride`) that a plain streaming window ships to the host: its owned samples + the tail of utterances that end in it
    void copy_span(size_t w, size_t stride, size_t& g0, size_t& g1) const {
        g0 = (size_t)chunk_begin(w);
        g1 = std::min(stride, (size_t)wins[w].f1 * M + (size_t)sadd[n_up]);
    }

    // ---- tables ----
    // the device table [window][n_up + 2][B] of a windowed call: the stage lengths of each utterance inside the window, then its emit end
    size_t table_rows() const { return (size_t)n_up + 2; }
    std::vector<int> device_table() const;
    // [window][2][B]: per utterance [what was final before w, what is final after it) in final_of's unit: final_of(b, e) = what is final of utterance b once
    // its model-rate samples [0, e) are (monotone in e). A window that finalises nothing for an utterance holds an empty range there.
    void range_table(std::vector<int>& table, const std::function<int(int, int64_t)>& final_of) const;
};

}  // namespace vits
