// delivery_plan.h — how a call's PCM travels from the vocoder to what is handed out (host only, like launch_plan.h and tile_map.h: no kernel, no device).
// The stages behind the vocoder — a stated tempo (tempo.hip), a stated pitch (pitch.hip), stated edges (edges.hip), level or limiter (loudness.hip, limiter.hip), output rate (resample.hip) — each read what the
// stage in front of them wrote. delivery_plan() states that chain ONCE, from what the handle and the call ask for: who runs, which buffer each stage reads
// and writes, which buffer is delivered, which arena buffers the call therefore needs, or why the combination is refused. The plan is ONE array in chain order,
// DeliveryPlan::stage[STAGE_COUNT]; the engine keeps what it knows of the rows behind every stage in an array of the same order (Call::behind), allocates from
// the plan (layout_stage_two) and resolves its buffer and stride ids to pointers and numbers in one place (Call::rows_of). tests/delivery_plan_dump.cpp prints
// the plan of every ask; the four tables tests/golden/{delivery,joined,pitch,tempo}_plan_table.txt pin it.
#pragma once

namespace vits {

// the closed set of buffers a stage can read or write; every buffer has one row stride (DeliveryStride)
enum DeliveryBuf : int {
    BUF_NONE = 0,  // nothing: the vocoder's source, the destination of a level that only measures
    BUF_WAVE,      // s2.wave: the vocoder's waveform [B][S_stride]
    BUF_EDGE,      // s2.wave_edge: the edges stage's output [B][E_stride]
    BUF_LVL,       // s2.wave_lvl: the levelled (or limited) waveform, rows as long as its input's
    BUF_OUT,       // s2.wave_out: the PCM at the output rate [B][out_ws]
    BUF_CALLER,    // opts.out_device, rows out_device_stride apart
    BUF_JOIN,      // s2.wave_join: the joined tracks [G][J_stride] (a joined ask only)
    BUF_PITCH,     // s2.wave_pitch: the varispeed rows [B][P_stride] (an ask with pitch only)
    BUF_TEMPO,     // s2.wave_tempo: the time-stretched rows [B][T_stride] (an ask with tempo only)
    BUF_COUNT
};
enum DeliveryStride : int {
    STRIDE_NONE = 0,
    STRIDE_S,       // S_stride: the vocoder's rows
    STRIDE_E,       // E_stride: the model-rate rows behind the edges stage (the bounds N + Pl + Pt)
    STRIDE_OUT_WS,  // out_ws: the rows at the output rate
    STRIDE_CALLER,  // out_device_stride
    STRIDE_J,       // J_stride: the model-rate rows behind the join, one per track (the largest track bound; a joined ask only)
    STRIDE_P,       // P_stride: the rows behind the pitch stage, twice the stride of the rows in front of it (the bound of N' at the smallest ratio, 0.5): 2 S_stride,
                    // or behind the tempo stage 2 T_stride (an ask with pitch only)
    STRIDE_T,       // T_stride = 2 S_stride: the rows behind the tempo stage (the bound of N' at the smallest tempo, 0.5; an ask with tempo only)
    STRIDE_COUNT
};
// the level kinds as delivery sees them. The kinds that multiply are two here because only a plain gain streams
enum DeliveryLevel : int {
    DLEVEL_NONE = 0,
    DLEVEL_MEASURE,  // VITS_LEVEL_MEASURE: reads, writes nothing
    DLEVEL_GAIN,     // VITS_LEVEL_GAIN
    DLEVEL_WHOLE,    // VITS_LEVEL_PEAK, VITS_LEVEL_LOUDNESS: the gain is known once the whole utterance is
    DLEVEL_COUNT
};
enum DeliveryRefusal : int {
    DELIVER_OK = 0,
    REFUSE_LIMIT_STREAM,  // on_chunk with the limiter on and a level that multiplies
    REFUSE_LEVEL_STREAM,  // on_chunk with a level that needs the whole utterance
    REFUSE_EDGES_STREAM,  // on_chunk with the edges stage on
    REFUSE_EDGES_ASYNC,   // async with the edges stage on
    REFUSE_JOIN_STREAM,   // a joined ask with on_chunk: no sample of a track is final before its last utterance is placed
    REFUSE_JOIN_ASYNC,    // a joined ask with async: the track lengths are read from the device behind the call's work
    REFUSE_PITCH_STREAM,  // pitch with on_chunk: streaming pitch is not built (a window's last samples need the next window's first)
    REFUSE_PITCH_ASYNC,   // pitch with async: the ratios travel through memory the call owns
    REFUSE_TEMPO_STREAM,  // tempo with on_chunk: where a segment starts is decided by the samples around it, which a window's end does not have yet
    REFUSE_COUNT
};
enum DeliveryNeed : unsigned {
    NEED_WAVE_EDGE = 1u << 0,
    NEED_WAVE_LVL = 1u << 1,
    NEED_WAVE_OUT = 1u << 2,
    NEED_ED_SCRATCH = 1u << 3,
    NEED_LVL_SCRATCH = 1u << 4,
    NEED_LIM_SCRATCH = 1u << 5,
    NEED_OUT_RANGES = 1u << 6,  // streaming at another rate: the output samples each window finalises
    NEED_LVL_RANGES = 1u << 7,  // streaming under a gain: the model-rate samples each window finalises
    NEED_WAVE_JOIN = 1u << 8,   // a joined ask, unless the join writes straight to out_device: the tracks [G][J_stride]
    NEED_JOIN_TABLE = 1u << 9,  // a joined ask: the table join.hip reads
    NEED_WAVE_PITCH = 1u << 10,  // an ask with pitch, unless the stage writes straight to out_device: the rows [B][P_stride]
    NEED_WAVE_TEMPO = 1u << 11,  // an ask with tempo, unless the stage writes straight to out_device: the rows [B][T_stride]
    NEED_COUNT = 12
};

struct DeliveryAsk {
    bool edges = false;        // the handle's edges stage is on
    int level = DLEVEL_NONE;   // DeliveryLevel of the handle's level kind
    bool limiter = false;      // the handle's limiter is on (it acts when the level multiplies)
    bool rate = false;         // an output rate is set
    bool out_device = false;   // opts.out_device
    bool on_chunk = false;     // opts.on_chunk
    bool async = false;        // opts.async
    bool pitch = false;        // some utterance of the call has a pitch ratio other than 1: the varispeed runs behind the vocoder, in front of the edges stage
    bool tempo = false;        // some utterance of the call (a voice conversion) has a tempo other than 1: the time stretch runs behind the vocoder, in front of the varispeed
    bool joined = false;       // the call lays its utterances end to end into tracks (vits_model_process_joined): the join runs behind the edges stage
};

struct DeliveryRoute {
    int buf = BUF_NONE, stride = STRIDE_NONE;
    bool operator==(const DeliveryRoute& o) const { return buf == o.buf && stride == o.stride; }
};

// the stages in chain order: each reads what the last stage in front of it that wrote left behind. The join (a joined ask only), the pitch stage (an ask with
// pitch only) and the tempo stage (an ask with tempo only) always write when they run; off, they leave the plan of every other ask what it always was.
enum DeliveryStage : int { STAGE_VOCODER = 0, STAGE_TEMPO, STAGE_PITCH, STAGE_EDGES, STAGE_JOIN, STAGE_LEVEL, STAGE_RESAMPLE, STAGE_COUNT };

struct DeliveryPlan {
    int refusal = DELIVER_OK;  // not DELIVER_OK: nothing else is set
    struct Stage {
        bool runs = false;
        DeliveryRoute src, dst;
        DeliveryRoute after;  // what the chain holds behind this stage: its dst, or (a stage that only reads) its src
    } stage[STAGE_COUNT];
    bool multiplies = false;  // the level stage writes (a plain multiply, or the limiter)
    bool limits = false;      // ... through the limiter
    DeliveryRoute delivered;  // what the call hands out: the destination of the last stage that writes
    unsigned needs = 0;       // DeliveryNeed bits
    bool need(unsigned bit) const { return (needs & bit) != 0; }
    const Stage& operator[](int s) const { return stage[s]; }
};

DeliveryPlan delivery_plan(const DeliveryAsk& ask);

}  // namespace vits
