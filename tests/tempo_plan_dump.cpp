// tempo_plan_dump — the tempo half of the delivery planner (vits.cpp_amd/csrc/delivery_plan.cpp, DeliveryAsk::tempo = true) over every combination of its
// ask, with pitch or without (a conversion is never joined), for tests/test_tempo_host.py. Linked with delivery_plan.o ALONE, like delivery_plan_dump. One line
// per combination:
//   pitch=P edges=E level=KIND limiter=L rate=R out_device=D on_chunk=C async=A : refuse WHY
//   pitch=P ... async=A : vocoder SRC>DST | tempo SRC>DST | pitch SRC>DST | edges SRC>DST | level SRC>DST | resample SRC>DST | deliver BUF/stride | needs a,b,...
// SRC and DST are BUF/stride (NONE/- for nothing); a stage that does not run prints "off"; no needs print "-".
#include <cstdio>
#include <string>

#include "../vits.cpp_amd/csrc/delivery_plan.h"

using namespace vits;

static const char* const kBuf[BUF_COUNT] = {"NONE", "WAVE", "EDGE", "LVL", "OUT", "CALLER", "JOIN", "PITCH", "TEMPO"};
static const char* const kStride[STRIDE_COUNT] = {"-", "S_stride", "E_stride", "out_ws", "caller", "J_stride", "P_stride", "T_stride"};
static const char* const kLevel[DLEVEL_COUNT] = {"none", "measure", "gain", "whole"};
static const char* const kRefusal[REFUSE_COUNT] = {"ok",          "limit_stream", "level_stream", "edges_stream", "edges_async",
                                                   "join_stream", "join_async",   "pitch_stream", "pitch_async", "tempo_stream"};
static const char* const kNeed[NEED_COUNT] = {"wave_edge",   "wave_lvl",   "wave_out",   "ed_scratch", "lvl_scratch", "lim_scratch",
                                              "out_ranges", "lvl_ranges", "wave_join",  "join_table", "wave_pitch", "wave_tempo"};

static std::string route(const DeliveryRoute& r) { return std::string(kBuf[r.buf]) + "/" + kStride[r.stride]; }

static void stage(const char* name, const DeliveryPlan::Stage& st) {
    if (st.runs) std::printf("%s %s>%s | ", name, route(st.src).c_str(), route(st.dst).c_str());
    else std::printf("%s off | ", name);
}

int main() {
    for (int pitch = 0; pitch < 2; ++pitch)
        for (int edges = 0; edges < 2; ++edges)
            for (int level = 0; level < DLEVEL_COUNT; ++level)
                for (int limiter = 0; limiter < 2; ++limiter)
                    for (int rate = 0; rate < 2; ++rate)
                        for (int od = 0; od < 2; ++od)
                            for (int oc = 0; oc < 2; ++oc)
                                for (int as = 0; as < 2; ++as) {
                                    DeliveryAsk a;
                                    a.edges = edges, a.level = level, a.limiter = limiter, a.rate = rate, a.out_device = od, a.on_chunk = oc, a.async = as;
                                    a.pitch = pitch, a.tempo = true;
                                    const DeliveryPlan p = delivery_plan(a);
                                    std::printf("pitch=%d edges=%d level=%s limiter=%d rate=%d out_device=%d on_chunk=%d async=%d : ", pitch, edges, kLevel[level],
                                                limiter, rate, od, oc, as);
                                    if (p.refusal) {
                                        std::printf("refuse %s\n", kRefusal[p.refusal]);
                                        continue;
                                    }
                                    stage("vocoder", p[STAGE_VOCODER]);
                                    stage("tempo", p.tempo);
                                    stage("pitch", p.pitch);
                                    stage("edges", p[STAGE_EDGES]);
                                    stage("level", p[STAGE_LEVEL]);
                                    stage("resample", p[STAGE_RESAMPLE]);
                                    std::printf("deliver %s | needs ", route(p.delivered).c_str());
                                    bool any = false;
                                    for (int i = 0; i < NEED_COUNT; ++i)
                                        if (p.need(1u << i)) {
                                            std::printf("%s%s", any ? "," : "", kNeed[i]);
                                            any = true;
                                        }
                                    std::printf("%s\n", any ? "" : "-");
                                }
    return 0;
}
