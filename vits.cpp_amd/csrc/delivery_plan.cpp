// delivery_plan.cpp — the delivery chain of a call as one pure function (delivery_plan.h). Host arithmetic only.
#include "delivery_plan.h"

namespace vits {

DeliveryPlan delivery_plan(const DeliveryAsk& a) {
    DeliveryPlan p;
    const bool multiplies = a.level >= DLEVEL_GAIN;
    // the refusals, in the order the engine has always checked them (level before edges, the limiter's first); a joined ask is refused for what it is first,
    // then an ask with tempo, then one with pitch
    if (a.joined && a.on_chunk) p.refusal = REFUSE_JOIN_STREAM;
    else if (a.joined && a.async) p.refusal = REFUSE_JOIN_ASYNC;
    else if (a.tempo && a.on_chunk) p.refusal = REFUSE_TEMPO_STREAM;  // (async: a conversion, the one caller with a tempo, is synchronous and says so itself)
    else if (a.pitch && a.on_chunk) p.refusal = REFUSE_PITCH_STREAM;
    else if (a.pitch && a.async) p.refusal = REFUSE_PITCH_ASYNC;
    else if (a.on_chunk && a.limiter && multiplies) p.refusal = REFUSE_LIMIT_STREAM;
    else if (a.on_chunk && (a.level == DLEVEL_MEASURE || a.level == DLEVEL_WHOLE)) p.refusal = REFUSE_LEVEL_STREAM;
    else if (a.edges && a.on_chunk) p.refusal = REFUSE_EDGES_STREAM;
    else if (a.edges && a.async) p.refusal = REFUSE_EDGES_ASYNC;
    if (p.refusal) return p;

    p.multiplies = multiplies;
    p.limits = multiplies && a.limiter;
    // The stages that write, in their order, each into its own arena buffer — except the last one, which writes straight to the caller's buffer when the
    // call has one. The model-rate rows behind the edges stage are E_stride apart; with the stage off they keep the stride of what is in front of it: the
    // pitch stage's, else the tempo stage's, else the vocoder's. Behind a join they are the tracks', J_stride apart. The row bounds, once: a tempo stage's rows
    // hold at most 2 S_stride samples (T_stride), a pitch stage's at most twice what lies in front of it (P_stride: 2 S_stride, or 2 T_stride behind a tempo stage).
    // in the order of DeliveryStage: vocoder, tempo, pitch, edges, join, level, resample
    const bool writes[STAGE_COUNT] = {true, a.tempo, a.pitch, a.edges, a.joined, multiplies, a.rate};
    const int own[STAGE_COUNT] = {BUF_WAVE, BUF_TEMPO, BUF_PITCH, BUF_EDGE, BUF_JOIN, BUF_LVL, BUF_OUT};
    const int head_stride = a.pitch ? STRIDE_P : (a.tempo ? STRIDE_T : STRIDE_S);
    const int own_stride[STAGE_COUNT] = {STRIDE_S, STRIDE_T, STRIDE_P, STRIDE_E, STRIDE_J, a.joined ? STRIDE_J : (a.edges ? STRIDE_E : head_stride), STRIDE_OUT_WS};
    int last = 0;
    for (int s = 0; s < STAGE_COUNT; ++s)
        if (writes[s]) last = s;
    DeliveryRoute cur;  // what the next stage reads
    for (int s = 0; s < STAGE_COUNT; ++s) {
        DeliveryPlan::Stage& st = p.stage[s];
        if (s == STAGE_LEVEL && a.level == DLEVEL_MEASURE) {
            // measured where it lies (out_device included): the chain passes by
            st.runs = true;
            st.src = st.after = cur;
            continue;
        }
        if (!writes[s]) continue;
        st.runs = true;
        st.src = cur;
        if (s == last && a.out_device) st.dst = DeliveryRoute{BUF_CALLER, STRIDE_CALLER};
        else st.dst = DeliveryRoute{own[s], own_stride[s]};
        cur = st.after = st.dst;
    }
    p.delivered = cur;

    for (const DeliveryPlan::Stage& st : p.stage)
        for (const int buf : {st.src.buf, st.dst.buf}) {
            if (buf == BUF_EDGE) p.needs |= NEED_WAVE_EDGE;
            if (buf == BUF_LVL) p.needs |= NEED_WAVE_LVL;
            if (buf == BUF_OUT) p.needs |= NEED_WAVE_OUT;
            if (buf == BUF_JOIN) p.needs |= NEED_WAVE_JOIN;
            if (buf == BUF_PITCH) p.needs |= NEED_WAVE_PITCH;
            if (buf == BUF_TEMPO) p.needs |= NEED_WAVE_TEMPO;
        }
    if (a.edges) p.needs |= NEED_ED_SCRATCH;
    if (a.level != DLEVEL_NONE) p.needs |= NEED_LVL_SCRATCH;
    if (p.limits) p.needs |= NEED_LIM_SCRATCH;
    if (a.rate && a.on_chunk) p.needs |= NEED_OUT_RANGES;
    if (multiplies && a.on_chunk) p.needs |= NEED_LVL_RANGES;
    if (a.joined) p.needs |= NEED_JOIN_TABLE;
    return p;
}

}  // namespace vits
