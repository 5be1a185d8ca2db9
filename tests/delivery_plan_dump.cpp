// delivery_plan_dump — the delivery planner (vits.cpp_amd/csrc/delivery_plan.cpp) over every combination of one slice of its ask, for the four frozen tables:
//   delivery_plan_dump base     tests/golden/delivery_plan_table.txt  (tests/test_delivery_plan_host.py): neither joined, pitch nor tempo
//   delivery_plan_dump joined   tests/golden/joined_plan_table.txt    (tests/test_joined_plan_host.py):   joined = 1
//   delivery_plan_dump pitch    tests/golden/pitch_plan_table.txt     (tests/test_pitch_host.py):         pitch = 1, joined or not
//   delivery_plan_dump tempo    tests/golden/tempo_plan_table.txt     (tests/test_tempo_host.py):         tempo = 1, with pitch or without
// Linked with delivery_plan.o ALONE: that the link succeeds is the proof that the planner needs no kernel and no device. One line per combination:
//   [extra=X ]edges=E level=KIND limiter=L rate=R out_device=D on_chunk=C async=A : refuse WHY
//   [extra=X ]edges=E ... async=A : STAGE SRC>DST | ... | deliver BUF/stride | needs a,b,...
// with the stage columns of the slice. SRC and DST are BUF/stride (NONE/- for nothing); a stage that does not run prints "off"; no needs print "-".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/delivery_plan.h"

using namespace vits;

// the tables' names of the planner's enums, in their order: one name per value, or this does not compile
template <int N, class T, int M>
constexpr const T (&names(const T (&a)[M]))[M] {
    static_assert(M == N, "a name for every value of the enum, no more and no less");
    return a;
}
static const char* const kBufNames[] = {"NONE", "WAVE", "EDGE", "LVL", "OUT", "CALLER", "JOIN", "PITCH", "TEMPO"};
static const char* const kStrideNames[] = {"-", "S_stride", "E_stride", "out_ws", "caller", "J_stride", "P_stride", "T_stride"};
static const char* const kLevelNames[] = {"none", "measure", "gain", "whole"};
static const char* const kRefusalNames[] = {"ok",          "limit_stream", "level_stream", "edges_stream", "edges_async",
                                            "join_stream", "join_async",   "pitch_stream", "pitch_async",  "tempo_stream"};
static const char* const kNeedNames[] = {"wave_edge",  "wave_lvl",   "wave_out",  "ed_scratch", "lvl_scratch", "lim_scratch",
                                         "out_ranges", "lvl_ranges", "wave_join", "join_table", "wave_pitch",  "wave_tempo"};
static const char* const kStageNames[] = {"vocoder", "tempo", "pitch", "edges", "join", "level", "resample"};
static const auto& kBuf = names<BUF_COUNT>(kBufNames);
static const auto& kStride = names<STRIDE_COUNT>(kStrideNames);
static const auto& kLevel = names<DLEVEL_COUNT>(kLevelNames);
static const auto& kRefusal = names<REFUSE_COUNT>(kRefusalNames);
static const auto& kNeed = names<NEED_COUNT>(kNeedNames);
static const auto& kStage = names<STAGE_COUNT>(kStageNames);
static_assert(DLEVEL_COUNT == 4, "main() takes the level from two bits of its counter");

// a slice of the ask space: the bit it fixes at 1, the bit it walks in front of the seven common ones (and prints first), the stage columns of its table
struct Slice {
    const char* name;
    bool DeliveryAsk::*fixed;
    bool DeliveryAsk::*extra;
    const char* extra_name;
    std::vector<int> stages;
};
static const Slice kSlices[] = {
    {"base", nullptr, nullptr, nullptr, {STAGE_VOCODER, STAGE_EDGES, STAGE_LEVEL, STAGE_RESAMPLE}},
    {"joined", &DeliveryAsk::joined, nullptr, nullptr, {STAGE_VOCODER, STAGE_EDGES, STAGE_JOIN, STAGE_LEVEL, STAGE_RESAMPLE}},
    {"pitch", &DeliveryAsk::pitch, &DeliveryAsk::joined, "joined", {STAGE_VOCODER, STAGE_PITCH, STAGE_EDGES, STAGE_JOIN, STAGE_LEVEL, STAGE_RESAMPLE}},
    {"tempo", &DeliveryAsk::tempo, &DeliveryAsk::pitch, "pitch", {STAGE_VOCODER, STAGE_TEMPO, STAGE_PITCH, STAGE_EDGES, STAGE_LEVEL, STAGE_RESAMPLE}},
};

static std::string route(const DeliveryRoute& r) { return std::string(kBuf[r.buf]) + "/" + kStride[r.stride]; }

static void line(const Slice& sl, const DeliveryAsk& a) {
    const DeliveryPlan p = delivery_plan(a);
    if (sl.extra) std::printf("%s=%d ", sl.extra_name, (int)(a.*sl.extra));
    std::printf("edges=%d level=%s limiter=%d rate=%d out_device=%d on_chunk=%d async=%d : ", (int)a.edges, kLevel[a.level], (int)a.limiter, (int)a.rate,
                (int)a.out_device, (int)a.on_chunk, (int)a.async);
    if (p.refusal) {
        std::printf("refuse %s\n", kRefusal[p.refusal]);
        return;
    }
    for (const int s : sl.stages) {
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

int main(int argc, char** argv) {
    const Slice* sl = nullptr;
    for (const Slice& s : kSlices)
        if (argc == 2 && !std::strcmp(argv[1], s.name)) sl = &s;
    if (!sl) {
        std::fprintf(stderr, "usage: delivery_plan_dump base|joined|pitch|tempo\n");
        return 2;
    }
    // the extra bit, then edges, the level (two bits), limiter, rate, out_device, on_chunk, async: the last one fastest
    for (int i = 0; i < (sl->extra ? 512 : 256); ++i) {
        DeliveryAsk a;
        if (sl->fixed) a.*sl->fixed = true;
        if (sl->extra) a.*sl->extra = (i >> 8) & 1;
        a.edges = (i >> 7) & 1, a.level = (i >> 5) & 3, a.limiter = (i >> 4) & 1, a.rate = (i >> 3) & 1;
        a.out_device = (i >> 2) & 1, a.on_chunk = (i >> 1) & 1, a.async = i & 1;
        line(*sl, a);
    }
    return 0;
}
