// speak_plan_dump — the host assembly of vits_model_speak (vits.cpp_amd/csrc/join_host.cpp speak_plan: the text cut into spans, the spans tokenised, the ones
// with ids laid out as the batch of one joined call) for tests/test_join_call_host.py. Linked with join_host.o ALONE: no kernel, no device, no model. The
// tokenizer is a toy with the shape of the model's (add_blank): an ASCII letter is the id 1 + its place in the alphabet, a blank (0) lies around every id,
// everything else is unknown and gives nothing; a '#' in a span is refused, to show that a tokenizer's refusal travels.
//   speak_plan_dump SENTENCE_GAP_MS PARAGRAPH_GAP_MS TRACK_PER_PARAGRAPH TEXT     (TEXT "--null": a NULL text)
// prints "refused: MESSAGE" (exit 1), or "batch B id_stride S" and one line per kept span: "span I track G gap MS len N ids a,b,c".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/kernels.h"

static bool toy_tokenize(void*, const std::string& span, std::vector<int32_t>& ids, std::string& err) {
    ids.clear();
    for (const char ch : span) {
        if (ch == '#') {
            err = "the toy tokenizer refuses '#'";
            return false;
        }
        const int c = ch | 32;
        if (c < 'a' || c > 'z' || (ch & 0x80)) continue;
        if (ids.empty()) ids.push_back(0);
        ids.push_back(1 + c - 'a');
        ids.push_back(0);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: speak_plan_dump SENTENCE_GAP_MS PARAGRAPH_GAP_MS TRACK_PER_PARAGRAPH TEXT\n");
        return 2;
    }
    const char* text = std::strcmp(argv[4], "--null") ? argv[4] : nullptr;
    vits::SpeakPlan p;
    std::string err;
    if (!vits::speak_plan(text, (float)std::atof(argv[1]), (float)std::atof(argv[2]), std::atoi(argv[3]) != 0, toy_tokenize, nullptr, p, err)) {
        std::printf("refused: %s\n", err.c_str());
        return 1;
    }
    std::printf("batch %d id_stride %d\n", p.batch, p.id_stride);
    for (int k = 0; k < p.batch; ++k) {
        std::printf("span %d track %d gap %g len %d ids ", p.index[(size_t)k], p.track[(size_t)k], (double)p.gap_ms[(size_t)k], p.id_lens[(size_t)k]);
        // (the whole row: what lies past the span's length must be 0)
        for (int t = 0; t < p.id_stride; ++t) std::printf("%s%d", t ? "," : "", p.ids[(size_t)k * p.id_stride + t]);
        std::printf("\n");
    }
    return 0;
}
