// delivery_plan_dump — the delivery planner (vits.cpp_amd/csrc/delivery_plan.cpp) over every combination of its ask, for tests/test_delivery_plan_host.py.
// Linked with delivery_plan.o ALONE: that the link succeeds is the proof that the planner needs no kernel and no device. One line per combination:
//   edges=E level=KIND limiter=L rate=R out_device=D on_chunk=C async=A : refuse WHY
//   edges=E ... async=A : vocoder SRC>DST | edges SRC>DST | level SRC>DST | resample SRC>DST | deliver BUF/stride | needs a,b,...
// SRC and DST are BUF/stride (NONE/- for nothing); a stage that does not run prints "off"; no needs print "-".
#include <cstdio>
#include <string>

#include "../vits.cpp_amd/csrc/delivery_plan.h"

using namespace vits;

// the table's names of the planner's enums, in their order
static const char* const kBuf[BUF_COUNT] = {"NONE", "WAVE", "EDGE", "LVL", "OUT", "CALLER"};
static const char* const kStride[STRIDE_COUNT] = {"-", "S_stride", "E_stride", "out_ws", "caller"};
static const char* const kLevel[DLEVEL_COUNT] = {"none", "measure", "gain", "whole"};
static const char* const kRefusal[REFUSE_COUNT] = {"ok", "limit_stream", "level_stream", "edges_stream", "edges_async"};
static const char* const kNeed[NEED_COUNT] = {"wave_edge", "wave_lvl", "wave_out", "ed_scratch", "lvl_scratch", "lim_scratch", "out_ranges", "lvl_ranges"};
static const char* const kStage[STAGE_COUNT] = {"vocoder", "edges", "level", "resample"};

static std::string route(const DeliveryRoute& r) { return std::string(kBuf[r.buf]) + "/" + kStride[r.stride]; }

int main() {
    for (int edges = 0; edges < 2; ++edges)
        for (int level = 0; level < DLEVEL_COUNT; ++level)
            for (int limiter = 0; limiter < 2; ++limiter)
                for (int rate = 0; rate < 2; ++rate)
                    for (int od = 0; od < 2; ++od)
                        for (int oc = 0; oc < 2; ++oc)
                            for (int as = 0; as < 2; ++as) {
                                DeliveryAsk a;
                                a.edges = edges, a.level = level, a.limiter = limiter, a.rate = rate, a.out_device = od, a.on_chunk = oc, a.async = as;
                                const DeliveryPlan p = delivery_plan(a);
                                std::printf("edges=%d level=%s limiter=%d rate=%d out_device=%d on_chunk=%d async=%d : ", edges, kLevel[level], limiter, rate, od,
                                            oc, as);
                                if (p.refusal) {
                                    std::printf("refuse %s\n", kRefusal[p.refusal]);
                                    continue;
                                }
                                for (int s = 0; s < STAGE_COUNT; ++s) {
                                    if (p[s].runs) std::printf("%s %s>%s | ", kStage[s], route(p[s].src).c_str(), route(p[s].dst).c_str());
                                    else std::printf("%s off | ", kStage[s]);
                                }
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
