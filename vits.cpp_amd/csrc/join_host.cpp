// join_host.cpp — the host side of joined tracks (include/vits.h "joined tracks"): the tracks, gaps and bounds of a call (vits_join_plan), the
// table join.hip reads, the definition evaluated sequentially (vits_join_host), and the sentence splitter (vits_split_sentences). No
// device call in here: every public function answers on a machine without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "kernels.h"

namespace vits {

namespace {
std::string fmt(float v) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%.9g", (double)v);
    return buf;
}
}  // namespace

bool join_plan(int rate, int batch, const int32_t* track, const float* gap_ms, JoinPlan& p, std::string& err) {
    if (rate < kResampleMinRate || rate > kResampleMaxRate) {
        err = "rate " + std::to_string(rate) + " Hz is outside [" + std::to_string(kResampleMinRate) + ", " + std::to_string(kResampleMaxRate) + "]";
        return false;
    }
    if (batch < 1 || batch > 65535) {
        err = "batch = " + std::to_string(batch) + " is outside [1, 65535]";
        return false;
    }
    JoinPlan q;
    q.rate = rate, q.batch = batch;
    q.gap.assign((size_t)batch, 0);
    q.first.push_back(0);
    for (int b = 0; b < batch; ++b) {
        const int32_t t = track ? track[b] : 0, prev = b ? (track ? track[b - 1] : 0) : 0;
        if (b == 0 && t != 0) {
            err = "track[0] = " + std::to_string(t) + ": the first utterance opens track 0";
            return false;
        }
        if (b > 0 && t != prev && t != prev + 1) {
            err = "track[" + std::to_string(b) + "] = " + std::to_string(t) + " after track[" + std::to_string(b - 1) + "] = " + std::to_string(prev) +
                  ": the utterances of a track are consecutive and in order (each step is 0 or 1)";
            return false;
        }
        const bool opens = b == 0 || t != prev;
        if (opens && b > 0) q.first.push_back(b);
        const float ms = gap_ms ? gap_ms[b] : 0.f;
        if (!(std::isfinite(ms) && ms >= kJoinMinGapMs && ms <= kJoinMaxGapMs)) {
            err = "gap_ms[" + std::to_string(b) + "] = " + fmt(ms) + " (utterance " + std::to_string(b) + "): must be finite and in [-2000, 60000] ms";
            return false;
        }
        // samples(ms) of the edges definition, with the sign kept apart
        const int64_t mag = (int64_t)std::floor(std::fabs((double)ms) * rate / 1000 + 0.5);
        q.gap[(size_t)b] = opens ? 0 : (ms < 0.f ? -mag : mag);
    }
    q.first.push_back(batch);
    q.tracks = (int)q.first.size() - 1;
    // (a track whose pauses alone pass the limit is refused here, before a caller has made any audio for it)
    for (int g = 0; g < q.tracks; ++g) {
        int64_t pauses = 0;
        for (int b = q.first[(size_t)g]; b < q.first[(size_t)g + 1]; ++b) pauses += std::max<int64_t>(q.gap[(size_t)b], 0);
        if (pauses > kEdgesMaxLen) {
            err = "track " + std::to_string(g) + " (utterances " + std::to_string(q.first[(size_t)g]) + " .. " + std::to_string(q.first[(size_t)g + 1] - 1) +
                  ") has a bound of at least " + std::to_string(pauses) + " samples (its pauses alone), above the " + std::to_string(kEdgesMaxLen) +
                  " a track may have: split it into several tracks or calls";
            return false;
        }
    }
    p = std::move(q);
    return true;
}

bool join_bounds(JoinPlan& p, const int64_t* utt_bounds, std::string& err) {
    std::vector<int64_t> ub((size_t)p.batch), tb((size_t)p.tracks, 0);
    int64_t mu = 0, mt = 0;
    for (int g = 0; g < p.tracks; ++g) {
        for (int b = p.first[(size_t)g]; b < p.first[(size_t)g + 1]; ++b) {
            const int64_t n = utt_bounds[b];
            if (n < 0 || n > kEdgesMaxLen) {
                err = "utterance " + std::to_string(b) + " has a bound of " + std::to_string(n) + " samples: outside [0, " + std::to_string(kEdgesMaxLen) + "]";
                return false;
            }
            ub[(size_t)b] = n;
            mu = std::max(mu, n);
            tb[(size_t)g] += n + std::max<int64_t>(p.gap[(size_t)b], 0);  // (at most 65535 (2^30 + 2^24) < 2^47)
        }
        if (tb[(size_t)g] > kEdgesMaxLen) {
            err = "track " + std::to_string(g) + " (utterances " + std::to_string(p.first[(size_t)g]) + " .. " + std::to_string(p.first[(size_t)g + 1] - 1) + ") has a bound of " +
                  std::to_string(tb[(size_t)g]) + " samples, above the " + std::to_string(kEdgesMaxLen) + " a track may have: split it into several tracks or calls";
            return false;
        }
        mt = std::max(mt, tb[(size_t)g]);
    }
    p.ubound = std::move(ub), p.bound = std::move(tb);
    p.max_ubound = mu, p.max_bound = mt;
    return true;
}

std::vector<int64_t> join_table(const JoinPlan& p) {
    std::vector<int64_t> t(join_table_elems(p.batch, p.tracks));
    for (int b = 0; b < p.batch; ++b) t[(size_t)2 * b] = p.gap[(size_t)b], t[(size_t)2 * b + 1] = p.ubound[(size_t)b];
    int64_t* tr = t.data() + (size_t)2 * p.batch;
    for (int g = 0; g < p.tracks; ++g) tr[3 * g] = p.first[(size_t)g], tr[3 * g + 1] = p.first[(size_t)g + 1], tr[3 * g + 2] = p.bound[(size_t)g];
    return t;
}

void join_host(const JoinPlan& p, const float* x, int64_t x_stride, const int64_t* lens, float* y, int64_t y_stride, int64_t* track_lens, int64_t* rows) {
    for (int g = 0; g < p.tracks; ++g) {
        float* yr = y ? y + (int64_t)g * y_stride : nullptr;
        if (yr)
            for (int64_t j = 0; j < p.bound[(size_t)g]; ++j) yr[j] = 0.f;
        int64_t o = 0, n_prev = 0, e_prev = 0;
        for (int b = p.first[(size_t)g]; b < p.first[(size_t)g + 1]; ++b) {
            const int64_t n = std::min(std::max<int64_t>(lens[b], 0), p.ubound[(size_t)b]);
            if (b > p.first[(size_t)g]) {
                const int64_t gb = p.gap[(size_t)b];
                o += n_prev + (gb >= 0 ? gb : -std::min(-gb, std::min(n_prev / 2, n / 2)));
            }
            if (rows) rows[(size_t)2 * b] = o, rows[(size_t)2 * b + 1] = n;
            const float* xr = x ? x + (int64_t)b * x_stride : nullptr;
            if (yr)  // (below e_prev the predecessor has written: the one add; at and above it nobody has)
                for (int64_t k = 0; k < n; ++k) yr[o + k] = o + k < e_prev ? yr[o + k] + xr[k] : xr[k];
            n_prev = n, e_prev = o + n;
        }
        if (track_lens) track_lens[g] = e_prev;
    }
}

// ---- vits_split_sentences ---------------------------------------------------------------------------------------------------------------------------------
namespace {
inline bool ascii_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
// U+3002, U+FF01, U+FF1F in UTF-8
inline bool cjk_stop(const char* s, size_t i, size_t n) {
    if (i + 3 > n) return false;
    const unsigned char a = (unsigned char)s[i], b = (unsigned char)s[i + 1], c = (unsigned char)s[i + 2];
    return (a == 0xE3 && b == 0x80 && c == 0x82) || (a == 0xEF && b == 0xBC && (c == 0x81 || c == 0x9F));
}
}  // namespace

int64_t split_sentences(const char* text, int64_t* starts, int64_t* ends, int32_t* kinds, size_t cap) {
    const size_t n = std::strlen(text);
    int64_t count = 0;
    size_t s0 = 0;  // where the span being read begins
    // the span [s0, e) ends here; `next` is where the following one begins
    auto close = [&](size_t e, size_t next) {
        size_t a = s0, b = e;
        while (a < b && ascii_space((unsigned char)text[a])) ++a;
        while (b > a && ascii_space((unsigned char)text[b - 1])) --b;
        // (a span of terminators and whitespace alone says nothing: it counts as empty)
        bool content = false;
        for (size_t k = a; k < b && !content;) {
            const unsigned char c = (unsigned char)text[k];
            if (c == '.' || c == '!' || c == '?' || ascii_space(c)) ++k;
            else if (cjk_stop(text, k, n)) k += 3;
            else content = true;
        }
        if (content) {
            if ((size_t)count < cap) {
                if (starts) starts[count] = (int64_t)a;
                if (ends) ends[count] = (int64_t)b;
                if (kinds) kinds[count] = 0;
            }
            ++count;
        }
        s0 = next;
    };
    size_t i = 0;
    while (i < n) {
        const unsigned char c = (unsigned char)text[i];
        if (c == '.' || c == '!' || c == '?') {
            size_t j = i;
            while (j < n && (text[j] == '.' || text[j] == '!' || text[j] == '?')) ++j;
            if (j < n && ascii_space((unsigned char)text[j])) close(j, j);
            i = j;
        } else if (cjk_stop(text, i, n)) {
            close(i + 3, i + 3);
            i += 3;
        } else if (ascii_space(c)) {
            // a whitespace run with two or more newlines ends a paragraph: the span in front of it closes (if it has not), and is of kind 1
            size_t j = i, nl = 0;
            while (j < n && ascii_space((unsigned char)text[j])) nl += text[j++] == '\n';
            if (nl >= 2) {
                close(i, j);
                // (the last span in front of the run, whether this run or a terminator closed it)
                if (count > 0 && (size_t)(count - 1) < cap && kinds) kinds[count - 1] = 1;
            }
            i = j;
        } else ++i;
    }
    close(n, n);
    return count;
}

// ---- vits_model_speak: spans, kinds and gaps -> the batch of one joined call --------------------------------------------------------------------------------
bool speak_plan(const char* text, float sentence_gap_ms, float paragraph_gap_ms, bool track_per_paragraph, SpeakTokenize tokenize, void* user, SpeakPlan& p,
                std::string& err) {
    if (!text || !*text) {
        err = "the text is NULL or empty";
        return false;
    }
    for (const auto& [ms, name] : {std::make_pair(sentence_gap_ms, "sentence_gap_ms"), std::make_pair(paragraph_gap_ms, "paragraph_gap_ms")})
        if (!(std::isfinite(ms) && ms >= kJoinMinGapMs && ms <= kJoinMaxGapMs)) {
            err = std::string(name) + " = " + fmt(ms) + ": must be finite and in [-2000, 60000] ms";
            return false;
        }
    const int64_t n = split_sentences(text, nullptr, nullptr, nullptr, 0);
    std::vector<int64_t> starts((size_t)n), ends((size_t)n);
    std::vector<int32_t> kinds((size_t)n);
    split_sentences(text, starts.data(), ends.data(), kinds.data(), (size_t)n);
    SpeakPlan q;
    std::vector<std::vector<int32_t>> kept;
    std::vector<char> ends_paragraph;  // [kept]
    for (int64_t i = 0; i < n; ++i) {
        std::vector<int32_t> ids;
        if (!tokenize(user, std::string(text + starts[(size_t)i], (size_t)(ends[(size_t)i] - starts[(size_t)i])), ids, err)) return false;
        if (ids.size() > (size_t)kSpeakMaxIds) {
            err = "span " + std::to_string(i) + " (bytes " + std::to_string(starts[(size_t)i]) + " .. " + std::to_string(ends[(size_t)i]) + ") has " +
                  std::to_string(ids.size()) + " ids, above the " + std::to_string(kSpeakMaxIds) + " an utterance may have: break the sentence up";
            return false;
        }
        if (ids.empty()) {
            // nothing to say: dropped; the paragraph it ended ends with the span in front of it
            if (kinds[(size_t)i] == 1 && !kept.empty()) ends_paragraph.back() = 1;
            continue;
        }
        q.id_stride = std::max(q.id_stride, (int)ids.size());
        q.index.push_back((int32_t)i);
        kept.push_back(std::move(ids));
        ends_paragraph.push_back(kinds[(size_t)i] == 1);
    }
    if (kept.empty()) {
        err = "no speakable span: the text holds " + std::to_string(n) + " span" + (n == 1 ? "" : "s") + " and none of them has a symbol the tokenizer knows";
        return false;
    }
    if (kept.size() > 65535) {
        err = "the text has " + std::to_string(kept.size()) + " speakable spans, above the 65535 a call may join: speak it in parts";
        return false;
    }
    q.batch = (int)kept.size();
    q.ids.assign((size_t)q.batch * q.id_stride, 0);
    int32_t track = 0;
    for (int k = 0; k < q.batch; ++k) {
        const bool new_paragraph = k > 0 && ends_paragraph[(size_t)k - 1];
        if (new_paragraph && track_per_paragraph) ++track;
        q.track.push_back(track);
        q.gap_ms.push_back(k == 0 ? 0.f : (new_paragraph ? paragraph_gap_ms : sentence_gap_ms));
        q.id_lens.push_back((int32_t)kept[(size_t)k].size());
        std::copy(kept[(size_t)k].begin(), kept[(size_t)k].end(), q.ids.begin() + (size_t)k * q.id_stride);
    }
    p = std::move(q);
    return true;
}

}  // namespace vits
