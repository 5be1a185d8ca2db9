// engine_voices.cpp — custom voices (include/vits.h vits_model_add_voices; DESIGN.md §8 "Custom voices"): speaker embeddings registered at run time.
// load_speakers folds the speaker terms of every conditioned conv into an effective-bias table with one row per file speaker; a voice is one more row of
// that table (and of the posterior encoder's, once conversion is prepared), computed from the caller's vector by the same 1x1 conditioning convs in the
// same order of operations (voices.hip). Voice k = id num_speakers + k = row 1 + num_speakers + k: the per-call row upload and the kernels are untouched.
#include <cmath>

#include "engine_internal.h"

namespace vits {

// the conditioning convs of one table uploaded for its first registration, with the segment descriptors of voices.hip: staged here, handed to the
// table only when the whole registration has succeeded (voice_rows)
struct Engine::VoiceResident {
    VoiceTable* t = nullptr;
    void* p[3] = {nullptr, nullptr, nullptr};  // weights [sum n][E], biases [sum n], descriptors
    size_t bytes = 0;
    int tiles = 0;
};

int Engine::voice_table_stage(VoiceTable& t, VoiceResident& r, std::string& err) {
    const int E = hp.speaker_embedding_size;
    std::vector<VoiceSeg> segs;
    const size_t bytes[3] = {t.cond_w.size() * sizeof(float), t.cond_b.size() * sizeof(float), t.segs.size() * sizeof(VoiceSeg)};
    bool ok = !t.segs.empty() && !t.cond_w.empty();
    for (int i = 0; i < 3 && ok; ++i) ok = hipMalloc(&r.p[i], bytes[i]) == hipSuccess;
    if (ok) {
        int64_t row = 0;
        for (const VoiceTable::Seg& s : t.segs) {
            segs.push_back({(const float*)r.p[0] + row * E, (const float*)r.p[1] + row, s.off, s.n, r.tiles});
            r.tiles += voice_seg_tiles(s.n);
            row += s.n;
        }
        ok = hipMemcpy(r.p[0], t.cond_w.data(), bytes[0], hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(r.p[1], t.cond_b.data(), bytes[1], hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(r.p[2], segs.data(), bytes[2], hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        for (void*& q : r.p) {
            if (q) hipFree(q);
            q = nullptr;
        }
        err = "hipMalloc failed for the resident conditioning convs of the voice registry (the registry keeps what it had)";
        return -1;
    }
    r.t = &t;
    r.bytes = bytes[0] + bytes[1] + bytes[2];
    return 0;
}

int Engine::voice_rows(const std::vector<VoiceTable*>& tabs, const float* emb, int n, int row_first, std::string& err) {
    const int E = hp.speaker_embedding_size, N = hp.num_speakers;
    if (front_) HIP_OK(hipStreamSynchronize(front_));
    HIP_OK(hipStreamSynchronize(stream));  // nothing in flight reads a table that is about to move
    async_tail_ = false;
    // everything the call allocates is staged first and handed over at the end: on any failure the handle is as it was
    struct Grown {
        VoiceTable* t;
        float* fresh;
        int cap;
    };
    std::vector<VoiceResident> resident;
    std::vector<Grown> grown;
    float* d_emb = nullptr;
    auto drop = [&]() {
        for (VoiceResident& r : resident)
            for (void* q : r.p)
                if (q) hipFree(q);
        for (Grown& g : grown) hipFree(g.fresh);
        if (d_emb) hipFree(d_emb);
    };
    const int need = row_first + n;
    for (VoiceTable* t : tabs) {
        if (row_first > t->cap_rows) {
            drop();
            err = "voice registry: table rows out of order";
            return -1;
        }
        if (!t->d_segs) {
            resident.emplace_back();
            if (voice_table_stage(*t, resident.back(), err)) {
                resident.pop_back();
                drop();
                return -1;
            }
        }
        if (need <= t->cap_rows) continue;
        const int cap = std::max(need, 1 + N + 2 * (t->cap_rows - 1 - N));  // capacity doubling, counted in voices
        float* fresh = nullptr;
        if (hipMalloc((void**)&fresh, (size_t)cap * t->rs * sizeof(float)) != hipSuccess) {
            drop();
            err = "hipMalloc failed for " + std::to_string(cap) + " rows of the effective-bias table (the voice registry keeps what it had)";
            return -1;
        }
        grown.push_back({t, fresh, cap});
    }
    if (hipMalloc((void**)&d_emb, (size_t)n * E * sizeof(float)) != hipSuccess) {
        drop();
        err = "hipMalloc failed for the staging copy of " + std::to_string(n) + " voice embeddings (the voice registry keeps what it had)";
        return -1;
    }
    prof.fence();
    bool ok = hipMemcpyAsync(d_emb, emb, (size_t)n * E * sizeof(float), hipMemcpyHostToDevice, stream) == hipSuccess;
    for (Grown& g : grown)
        ok = ok && hipMemcpyAsync(g.fresh, g.t->table, (size_t)row_first * g.t->rs * sizeof(float), hipMemcpyDeviceToDevice, stream) == hipSuccess;
    for (VoiceTable* t : tabs) {
        float* dst = t->table;
        const VoiceSeg* segs = t->d_segs;
        int tiles = t->tiles;
        for (Grown& g : grown)
            if (g.t == t) dst = g.fresh;
        for (VoiceResident& r : resident)
            if (r.t == t) segs = (const VoiceSeg*)r.p[2], tiles = r.tiles;
        ok = ok && launch_voice_rows(segs, (int)t->segs.size(), tiles, d_emb, n, E, dst, t->rs, row_first, stream) == hipSuccess;
    }
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    if (!ok) {
        drop();
        err = "could not build the voices' rows of the effective-bias table on the device";
        return -1;
    }
    hipFree(d_emb);
    for (VoiceResident& r : resident) {
        VoiceTable& t = *r.t;
        t.d_w = (float*)r.p[0], t.d_b = (float*)r.p[1], t.d_segs = (VoiceSeg*)r.p[2];
        t.tiles = r.tiles;
        for (void* q : r.p) owned_.push_back(q);
        weight_bytes += (int64_t)r.bytes;
        std::vector<float>().swap(t.cond_w);  // (the device copy is the one that is read from here on)
        std::vector<float>().swap(t.cond_b);
    }
    for (Grown& g : grown) {
        VoiceTable& t = *g.t;
        for (void*& p : owned_)
            if (p == t.table) p = g.fresh;
        hipFree(t.table);
        weight_bytes += (int64_t)(g.cap - t.cap_rows) * t.rs * (int64_t)sizeof(float);
        t.table = g.fresh;
        t.cap_rows = g.cap;
        for (VoiceTable::Seg& s : t.segs) s.pc->bias = t.table + s.off;  // (bias_rs stays: the row stride does not change)
    }
    return 0;
}

namespace {
// 0, or -1 + a message naming the voice and the element of the first value that is not finite
int check_finite(const float* emb, int n, int E, int first_id, std::string& err) {
    for (int v = 0; v < n; ++v)
        for (int e = 0; e < E; ++e)
            if (!std::isfinite(emb[(size_t)v * E + e])) {
                err = "voice " + std::to_string(v) + " (id " + std::to_string(first_id + v) + "), element " + std::to_string(e) + " is not finite";
                return -1;
            }
    return 0;
}
}  // namespace

int Engine::add_voices(const float* emb, int n, int32_t* ids_out, std::string& err) {
    const int E = hp.speaker_embedding_size, N = hp.num_speakers, nv = num_voices();
    if (N <= 1 || !vt_main_.table) {
        err = "vits_model_add_voices: this model has a single speaker and no speaker conditioning";
        return -1;
    }
    if (n <= 0) {
        err = "vits_model_add_voices: n = " + std::to_string(n) + " (at least one voice)";
        return -1;
    }
    if ((int64_t)N + nv + n > (int64_t)1 << 24) {
        err = "vits_model_add_voices: more than 2^24 speakers and voices";
        return -1;
    }
    if (check_finite(emb, n, E, N + nv, err)) return -1;
    std::vector<VoiceTable*> tabs{&vt_main_};
    if (vt_post_.table) tabs.push_back(&vt_post_);
    if (voice_rows(tabs, emb, n, 1 + N + nv, err)) return -1;
    voices_.insert(voices_.end(), emb, emb + (size_t)n * E);
    for (int v = 0; v < n; ++v) ids_out[v] = N + nv + v;
    return 0;
}

int Engine::set_voice(int id, const float* emb, std::string& err) {
    const int E = hp.speaker_embedding_size, N = hp.num_speakers, nv = num_voices();
    if (N <= 1) {
        err = "vits_model_set_voice: this model has a single speaker and no speaker conditioning";
        return -1;
    }
    if (id < N || id >= N + nv) {
        err = "vits_model_set_voice(" + std::to_string(id) + "): not a registered voice (voices are the ids [" + std::to_string(N) + ", " + std::to_string(N + nv) + "))";
        return -1;
    }
    if (check_finite(emb, 1, E, id, err)) return -1;
    std::vector<VoiceTable*> tabs{&vt_main_};
    if (vt_post_.table) tabs.push_back(&vt_post_);
    if (voice_rows(tabs, emb, 1, 1 + id, err)) return -1;
    std::copy(emb, emb + E, voices_.begin() + (size_t)(id - N) * E);
    return 0;
}

int Engine::clear_voices(std::string& err) {
    if (hp.num_speakers <= 1) {
        err = "vits_model_clear_voices: this model has a single speaker and no speaker conditioning";
        return -1;
    }
    if (speaker >= hp.num_speakers) {
        err = "vits_model_clear_voices: the model's default speaker " + std::to_string(speaker) + " is a voice (vits_model_set_speaker to -1 or a file speaker first)";
        return -1;
    }
    voices_.clear();  // (the tables keep their rows and the convs stay resident: the next registration reuses both)
    return 0;
}

int Engine::get_speaker_embedding(int id, float* dst, size_t cap, std::string& err) const {
    const int E = hp.speaker_embedding_size, N = hp.num_speakers;
    if (N <= 1) {
        err = "vits_model_get_speaker_embedding: this model has a single speaker and no speaker embedding";
        return -1;
    }
    if (id < 0 || id >= speaker_limit()) {
        err = "vits_model_get_speaker_embedding(" + std::to_string(id) + "): neither a speaker of the file nor a registered voice (ids [0, " +
              std::to_string(speaker_limit()) + "))";
        return -1;
    }
    const float* src = id < N ? spk_emb_.data() + (size_t)id * E : voices_.data() + (size_t)(id - N) * E;
    std::copy(src, src + std::min<size_t>(cap, (size_t)E), dst);
    return E;
}

}  // namespace vits
