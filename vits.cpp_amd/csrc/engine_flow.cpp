// engine_flow.cpp — stage two of a call up to the vocoder: arena layout (sized by B x L after the host read of the frame
// counts), prior sampling through the alignment (vits.cpp:1028-1064) and the residual coupling flow, reverse
// (vits.cpp:519-538,500-517,452-498).
#include <thread>

#include "engine_internal.h"

namespace vits {

int Engine::layout_stage_two(Call& c) {
    const vits_process_opts& o = c.o;
    const int B = c.B, n_up = c.n_up;
    const int H = hp.hidden, F = hp.flow_size;
    const int Lmax = c.Lmax;
    Call::S2& s2 = c.s2;
    const WindowPlan& wins = c.win;
    const bool windowed = wins.windowed;
    const int Lw_max = wins.Lw_max;
    const std::vector<int>& smul = c.smul;
    const std::vector<int>& sadd = c.sadd;
    // ---- stage two buffers -------------------------------------------------------------------------------------
    const int ls = c.ls = round_up(Lmax, 32), lws = c.lws = round_up(Lw_max, 32);
    size_t& big = c.big;
    big = 0;
    std::vector<int>& sts = c.sts;
    sts.assign(n_up + 1, 0);
    for (int i = 0; i <= n_up; ++i) sts[i] = round_up(Lw_max * smul[i] + sadd[i], 32);
    for (int i = 0; i < n_up; ++i) big = std::max(big, (size_t)B * ups_[i].channels * sts[i + 1]);
    const bool need_noise_buf = o.noise_kind != VITS_NOISE_COUNTER;
    // 16-bit arithmetic modes: the vocoder runs in the group layout of conv16.hip when its channel counts allow it (with or without
    // collect_taps: every tap is a tensor both layouts produce in fp32 [c][t]); scratch for the converter path's rounded inputs
    const bool fast16 = c.fast16 = arith_now_ != VITS_ARITH_F32 && vocoder_group_ok_ && !knobs.no_group16;
    c.fuse16 = fast16 && !knobs.no_fuse16;  // resblock conv pairs of the narrow stages as one kernel
    const size_t x16_elems2 = arith_now_ != VITS_ARITH_F32 ? std::max({big, (size_t)B * round_up(H, 8) * round_up(ls, 8), (size_t)B * round_up(hp.up_init, 8) * round_up(lws, 8), (size_t)B * round_up(F, 8) * round_up(ls, 8)}) + 64 : 0;
    // the delivery chain: the rows behind every stage (Call::behind, filled by Engine::plan_rows) and the plan's routes size its buffers. R: the rows behind the
    // join, one per utterance or — a joined call — one per track
    const DeliveryPlan& dp = c.dp;
    const Call::RowSet* const behind = c.behind;
    const int S_stride = behind[STAGE_VOCODER].stride;
    const int R = behind[STAGE_JOIN].n;
    // no stage writes a row longer than the stride of what it writes to: a wrong stride is refused here, on the host, before anything of stage two is queued
    static const char* const stage_name[STAGE_COUNT] = {"vocoder", "tempo", "pitch", "edges", "join", "level", "resample"};
    for (int s = 0; s < STAGE_COUNT; ++s) {
        const int64_t stride = c.rows_of(dp[s].dst).stride;  // (out_device: out_device_stride)
        if (dp[s].runs && dp[s].dst.buf != BUF_NONE && behind[s].max > stride) {
            c.err = std::string("delivery chain: the ") + stage_name[s] + " stage's longest row has " + std::to_string(behind[s].max) +
                    " samples, and the rows it writes are " + std::to_string(stride) + " apart";
            return -1;
        }
    }
    // VITS_ARITH_F32_SPLIT: three bf16 planes per conv input of the wide stages' resblocks (conv_split.hip): the stage input once, t and the stream per
    // concurrently running resblock
    size_t sp_elems = 0;
    if (split_on())
        for (int i = 0; i < n_up; ++i)
            if (ups_[i].channels >= 128 && ups_[i].channels % 32 == 0) sp_elems = std::max(sp_elems, (size_t)3 * B * ups_[i].channels * sts[i + 1] + 64);
    auto layout2 = [&](Arena& a) {
        s2.zp = a.alloc<float>((size_t)B * F * ls);
        s2.noise = need_noise_buf ? a.alloc<float>((size_t)B * F * ls) : nullptr;
        s2.hout = a.alloc<float>((size_t)B * 2 * H * ls);
        s2.gate = a.alloc<float>((size_t)B * H * ls);
        s2.h0 = a.alloc<float>((size_t)B * hp.up_init * lws);
        s2.win_lens = windowed ? a.alloc<int>(wins.size() * wins.table_rows() * B) : nullptr;
        s2.bu = a.alloc<float>(big);
        s2.bul = a.alloc<float>(big);
        for (int j = 0; j < 3; ++j) {
            // one (y, t) pair per concurrently running resblock
            const bool own = j == 0 || (knobs.rb_streams > 1 && (size_t)j < hp.rb_k.size());
            s2.by[j] = own ? a.alloc<float>(big) : s2.by[0];
            s2.bt[j] = own ? a.alloc<float>(big) : s2.bt[0];
            s2.byl[j] = own ? a.alloc<float>(big) : s2.byl[0];
        }
        s2.bs = a.alloc<float>(big);
        s2.bs16 = fast16 ? a.alloc<float>(big / 2 + 64) : nullptr;
        for (int j = 0; j < 3; ++j) s2.x16[j] = (x16_elems2 && (j == 0 || (knobs.rb_streams > 1 && !fast16))) ? a.alloc<uint16_t>(x16_elems2) : nullptr;
        s2.sp_u = sp_elems ? a.alloc<uint16_t>(sp_elems) : nullptr;
        for (int j = 0; j < 3; ++j) {
            const bool own = j == 0 || (knobs.rb_streams > 1 && (size_t)j < hp.rb_k.size());
            s2.sp_t[j] = !sp_elems ? nullptr : (own ? a.alloc<uint16_t>(sp_elems) : s2.sp_t[0]);
            s2.sp_y[j] = !sp_elems ? nullptr : (own ? a.alloc<uint16_t>(sp_elems) : s2.sp_y[0]);
        }
        s2.pre = o.collect_taps ? a.alloc<float>((size_t)B * S_stride) : nullptr;
        s2.wave = a.alloc<float>((size_t)B * S_stride);
        // the buffers of the delivery chain: exactly what the call's plan names (delivery_plan.h; a stage that writes straight to out_device needs none)
        s2.wave_out = dp.need(NEED_WAVE_OUT) ? a.alloc<float>((size_t)R * behind[STAGE_RESAMPLE].stride) : nullptr;
        s2.out_ranges = dp.need(NEED_OUT_RANGES) ? a.alloc<int>(wins.size() * (size_t)2 * B) : nullptr;
        s2.wave_lvl = dp.need(NEED_WAVE_LVL) ? a.alloc<float>((size_t)R * c.rows_of(dp[STAGE_LEVEL].dst).stride) : nullptr;  // (it follows its input's stride)
        s2.lvl_scratch = dp.need(NEED_LVL_SCRATCH) ? a.alloc<char>(level_scratch_bytes(R, behind[STAGE_LEVEL - 1].max, level_plan_.S)) : nullptr;
        s2.lim_scratch = dp.need(NEED_LIM_SCRATCH) ? a.alloc<char>(limit_scratch_bytes(R, behind[STAGE_LEVEL - 1].max)) : nullptr;
        s2.wave_edge = dp.need(NEED_WAVE_EDGE) ? a.alloc<float>((size_t)B * behind[STAGE_EDGES].stride) : nullptr;
        s2.ed_scratch = dp.need(NEED_ED_SCRATCH) ? a.alloc<char>(edges_scratch_bytes(B, behind[STAGE_EDGES - 1].max, edges_plan_.W)) : nullptr;
        s2.lvl_ranges = dp.need(NEED_LVL_RANGES) ? a.alloc<int>(wins.size() * (size_t)2 * B) : nullptr;
        s2.tile_maps = c.tm_total ? a.alloc<TileEntry>((size_t)c.tm_total) : nullptr;
        s2.wave_join = dp.need(NEED_WAVE_JOIN) ? a.alloc<float>((size_t)R * behind[STAGE_JOIN].stride) : nullptr;
        s2.join_table = dp.need(NEED_JOIN_TABLE) ? a.alloc<int64_t>(join_table_elems(B, R)) : nullptr;
        s2.wave_pitch = dp.need(NEED_WAVE_PITCH) ? a.alloc<float>((size_t)B * behind[STAGE_PITCH].stride) : nullptr;
        s2.pitch_ratios = dp[STAGE_PITCH].runs ? a.alloc<float>((size_t)B) : nullptr;
        s2.pitch_lens = dp[STAGE_PITCH].runs ? a.alloc<int>((size_t)B) : nullptr;
        s2.wave_tempo = dp.need(NEED_WAVE_TEMPO) ? a.alloc<float>((size_t)B * behind[STAGE_TEMPO].stride) : nullptr;
        s2.tempo_q = dp[STAGE_TEMPO].runs ? a.alloc<float>((size_t)B) : nullptr;
        s2.tempo_lens = dp[STAGE_TEMPO].runs ? a.alloc<int>((size_t)B) : nullptr;
        s2.tempo_starts = dp[STAGE_TEMPO].runs ? a.alloc<int>((size_t)B * (size_t)c.tem_starts) : nullptr;
    };
    if (arena_layout(a2_, stream, c.err, layout2)) return -1;
    set_x16_scratch(s2.x16[0], s2.x16[1], s2.x16[2], x16_elems2);
    for (int i = 0; i <= n_up && i < 8; ++i) c.d_len_full[i] = c.s1.stage_lens + (size_t)i * B;
    return 0;
}

// ---- prior sampling through the alignment (vits.cpp:1028-1064) -------------------------------------------
int Engine::run_prior_sampling(Call& c) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const int B = c.B, F = hp.flow_size;
    const std::vector<int>& frames = c.frames;
    const int Lmax = c.Lmax;
    Call::S1& s1 = c.s1;
    Call::S2& s2 = c.s2;
    auto TR = make_ref;
    auto sub = sub_rows;
    const int id_stride = c.id_stride, ls = c.ls;
    const int* dl = s1.lens;
    TensorRef stats = TR(s1.stats, 2 * F, c.ts);
    c.rx.phase("vits.prior_sampling");
    TensorRef zp = TR(s2.zp, F, ls), noise = TR(s2.noise, F, ls);
    if (c.ref_ahead) {
        // batch 1, reference noise: the tensor was (mostly) drawn while stage one ran (engine.cpp); it is one dense [F][L] block in pinned memory
        const int L = frames[0];
        const size_t n = (size_t)F * (size_t)L;
        PinnedBuf<float> block;  // a larger one; after the swap the old one, which goes only when the helper has moved over and finished
        if (n > ref_noise_pinned_.cap) {  // (more frames per id than the block was sized for: a larger block once the helper rests at the old capacity; keep what was drawn)
            while (c.ref_ahead->drawn() < c.ref_ahead->capacity()) std::this_thread::yield();
            HIP_OK(block.ensure(n, n));
            std::memcpy(block.p, ref_noise_pinned_.p, sizeof(float) * c.ref_ahead->drawn());
            ref_noise_pinned_.swap(block);
            c.ref_ahead->rebase(ref_noise_pinned_.p, ref_noise_pinned_.cap);
        }
        c.ref_ahead->finish(n);
        c.ref_ahead = nullptr;
        noise.cs = L;
        noise.bs = (int64_t)F * L;
        HIP_OK(hipMemcpyAsync(s2.noise, ref_noise_pinned_.p, sizeof(float) * n, hipMemcpyHostToDevice, stream));
        prof.fence();
        if (o.async) HIP_OK(hipStreamSynchronize(stream));  // (the pinned block is reused by the next call)
        if (o.collect_taps) snapshot("noise_prior", noise, F, Lmax, B, frames);
    } else if (o.noise_kind != VITS_NOISE_COUNTER && upload_host_noise(c))
        return -1;
    prof.begin("prior_sample_gather", 0, 0, stream);
    HIP_OK(launch_zp(sub(stats, 0), sub(stats, F), s1.cum, id_stride, dl, s1.frames, noise, o.noise_kind == VITS_NOISE_COUNTER ? VITS_NOISE_COUNTER : VITS_NOISE_EXPLICIT,
                     o.noise_seed, s1.seed_off, noise_scale, s1.noise_scale, zp, B, F, Lmax, stream));
    prof.end(stream);
    if (o.collect_taps) snapshot("z_p", zp, F, Lmax, B, frames);
    return 0;
}

// Host noise of every utterance (opts.noise_prior, or the reference stream: tensor_randn_like(prior_means ne=[L,F]), vits.cpp:1059, utterance by
// utterance) as [F][L] rows of s2.noise, and the noise_prior tap
int Engine::upload_host_noise(Call& c) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const int B = c.B, F = hp.flow_size, ls = c.ls;
    std::vector<float> hn((size_t)B * F * ls, 0.f);
    for (int b = 0; b < B; ++b) {
        const int L = c.frames[b];
        if (o.noise_kind == VITS_NOISE_EXPLICIT) {
            if (!o.noise_prior) {
                err = "noise_prior missing";
                return -1;
            }
            for (int ch = 0; ch < F; ++ch)
                std::memcpy(&hn[((size_t)b * F + ch) * ls], o.noise_prior + ((size_t)b * F + ch) * o.noise_prior_stride, sizeof(float) * std::min<int64_t>(L, o.noise_prior_stride));
        } else {
            std::vector<float> tmpn((size_t)F * L);
            reference_noise_fill(tmpn.data(), tmpn.size());
            for (int ch = 0; ch < F; ++ch) std::memcpy(&hn[((size_t)b * F + ch) * ls], &tmpn[(size_t)ch * L], sizeof(float) * L);
        }
    }
    HIP_OK(hipMemcpyAsync(c.s2.noise, hn.data(), sizeof(float) * hn.size(), hipMemcpyHostToDevice, stream));
    prof.fence();
    HIP_OK(hipStreamSynchronize(stream));  // hn goes out of scope
    if (o.collect_taps) snapshot("noise_prior", make_ref(c.s2.noise, F, ls), F, c.Lmax, B, c.frames);
    return 0;
}

// ---- one WaveNet stack (vits.cpp:452-498; transformers VitsWaveNet) -----------------------------------------------------------
int Engine::run_wavenet(Call& c, const std::vector<PackedConv>& in_layers, const std::vector<PackedConv>& res_skip, int n_layers, const WaveNetLabels& lab) {
    std::string& err = c.err;
    const int B = c.B, Lmax = c.Lmax, H = hp.hidden;
    const int64_t sum_frames = c.sum_frames;
    const int* ll = c.d_len_full[0];
    TensorRef hout = make_ref(c.s2.hout, 2 * H, c.ls), gate = make_ref(c.s2.gate, H, c.ls);
    TensorRef hh = hout, outputs = sub_rows(hout, H);  // channels [0,H) = h, [H,2H) = skip accumulator "outputs" (vits.cpp:460)
    auto mk = [&](TensorRef xin, TensorRef yout) {
        ConvCall k;
        k.x = xin;
        k.y = yout;
        k.len_in = ll;
        k.len_out = ll;
        k.spk = c.spk;  // (multi-speaker calls: read by the speaker-conditioned in_layers only)
        k.batch = B;
        k.t_in = k.t_out = Lmax;
        k.sum_in = k.sum_out = sum_frames;
        return k;
    };
    prof.begin("fill_zero", 0, 0, stream);
    HIP_OK(launch_fill_rows(outputs, H, 0.f, B, Lmax, stream));
    prof.end(stream);
    // Each layer as ONE kernel (wavenet32.hip; bit-identical to the two launches below). A fused block reads a
    // 2-frame halo of its neighbours' h columns, so h alternates between hout[0,H) and the buffer the two-launch path uses for the
    // gate output; `outputs` (hout[H,2H)) is updated in place.
    // (large grids only: at batch 1 a layer is four blocks, and a block's six waves on four SIMDs run two MFMA chains deep:
    // 68 us against 39 us for the two launches with their split-gate tiles)
    const bool f32 = arith_now_ == VITS_ARITH_F32;
    bool fuse = !knobs.no_wn_fuse && (c.ls & 3) == 0 && (int64_t)((Lmax + 31) / 32) * B >= 384 && (reinterpret_cast<uintptr_t>(hout.p) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(gate.p) & 15) == 0;
    for (int l = 0, dl = 1; l < n_layers && fuse; ++l, dl *= hp.wn_rate)
        fuse = (f32 ? wavenet32_supported(H, hp.wn_k, dl, in_layers[l], res_skip[l]) : wavenet16_supported(H, hp.wn_k, dl, in_layers[l], res_skip[l])) &&
               res_skip[l].cout == (l + 1 < n_layers ? 2 * H : H);
    TensorRef hcur = hh;
    for (int l = 0, dl = 1; l < n_layers; ++l, dl *= hp.wn_rate) {
        const PackedConv &in = in_layers[l], &rs = res_skip[l];
        const bool last = l + 1 == n_layers;
        if (fuse) {
            WaveNet32Call w;
            w.h = hcur;
            w.h_out = last ? TensorRef() : (hcur.p == gate.p ? hh : gate);
            w.outputs = outputs;
            w.lens = ll;
            w.spk = c.spk;
            w.batch = B;
            w.tmax = Lmax;
            w.hidden = H;
            w.dil = dl;  // (1: the fused kernels take no other, see *_supported)
            if (prof.on) {
                char full[160];
                std::snprintf(full, sizeof(full), "%s|k%d|d%d|%c%d|e1|c%dx%d", lab.layer, hp.wn_k, dl, f32 ? 'w' : 'W', H, H, rs.cout);
                prof.begin(full, 2.0 * ((double)2 * H * H * hp.wn_k + (double)rs.cout * H) * (double)sum_frames,
                           4.0 * (double)sum_frames * (H + 2.0 * rs.cout) + (double)in.bytes + (double)rs.bytes, stream, true);
            }
            if (f32) HIP_OK(launch_wavenet32(in, rs, w, stream));
            else HIP_OK(launch_wavenet16(in, rs, w, arith_now_, stream));
            prof.end(stream);
            if (w.h_out.p) hcur = w.h_out;
            continue;
        }
        ConvCall k = mk(hh, gate);
        k.dil = dl;
        k.pad_l = (hp.wn_k * dl - dl) / 2;  // vits.cpp:470
        HIP_OK(conv(lab.gated_conv, in, k));
        // all but the last layer: rows [0,H): h += res ; rows [H,2H): outputs += skip (vits.cpp:484-489); the last: outputs += res_skip (vits.cpp:491)
        ConvCall r = mk(gate, last ? outputs : hout);
        r.res = r.y;
        HIP_OK(conv(lab.conv1x1, rs, r));
    }
    return 0;
}

// ---- residual coupling flow, reverse (vits.cpp:519-538,500-517,452-498) ------------------------------------
// forward (voice conversion, transformers VitsResidualCouplingBlock.forward with reverse = False): layers 0 .. n-1, x1 += mean, through the
// same kernels with the not-negated conv_post packs (flow_fwd_post_). Layer i sees the same channel-flip parity (n - i) in both directions,
// so both read and write the one physical layout: the forward flow ends in the layout prior sampling writes z_p in.
int Engine::run_coupling(Call& c, bool forward) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const int B = c.B;
    const int H = hp.hidden, F = hp.flow_size;
    const std::vector<int>& frames = c.frames;
    const int Lmax = c.Lmax;
    auto sub = sub_rows;
    const int ls = c.ls;
    const int64_t sum_frames = c.sum_frames;
    TensorRef zp = make_ref(c.s2.zp, F, ls);
    c.rx.phase(forward ? "vits.flow_forward" : "vits.flow");
    const int* ll = c.d_len_full[0];
    TensorRef hout = make_ref(c.s2.hout, 2 * H, ls);
    const int* spk = c.spk;  // (multi-speaker calls: read by the speaker-conditioned in_layers only)
    auto mk2 = [&](TensorRef xin, TensorRef yout) {
        ConvCall c;
        c.x = xin;
        c.y = yout;
        c.len_in = ll;
        c.len_out = ll;
        c.spk = spk;
        c.batch = B;
        c.t_in = c.t_out = Lmax;
        c.sum_in = c.sum_out = sum_frames;
        return c;
    };
    // 16-bit modes, fused coupling layers: a layer is ONE launch of sum_b ceil(frames_b / 48) blocks, one block per CU at a time (238 VGPRs x six
    // waves) — 320 blocks at batch 64 x 225 frames = a full round on the 256 CUs and a second one on 64 of them, four times over. Utterances never
    // interact, so the batch is dealt out over two independent chains of launches (main stream + a side stream): while one chain's layer drains its
    // tail the other's blocks take the free CUs (4 x 320 blocks in ~5 rounds instead of 8). Same kernel, same operands per utterance: same bits.
    int chains = 1, chain_b0[3] = {0, B, B};
    bool all_fused = arith_now_ != VITS_ARITH_F32 && !knobs.no_flow_fuse;
    auto post_of = [&](int i) -> const PackedConv& { return forward ? flow_fwd_post_[i] : flow_[i].post; };
    for (int i = 0; i < hp.n_flows && all_fused; ++i)
        all_fused = (int)flow_[i].in_layers.size() == hp.wn_layers && (int)flow_[i].res_skip.size() == hp.wn_layers &&
                    flow_couple16_supported(H, F / 2, hp.wn_k, hp.wn_rate, hp.wn_layers, flow_[i].pre, flow_[i].in_layers.data(), flow_[i].res_skip.data(), post_of(i));
    if (all_fused && !prof.on && side_[0] && B >= 2 && knobs.flow_chains > 1) {
        int64_t blocks = 0;
        for (int b = 0; b < B; ++b) blocks += flow_wide_blocks(frames[b]);
        if (blocks > knobs.flow_chain_min_blocks && !flow_couple16_narrow(blocks)) {
            // equal shares of the blocks (by utterance, in order)
            int64_t run = 0;
            int cut = 0;
            while (cut < B - 1 && 2 * (run + flow_wide_blocks(frames[cut])) <= blocks) run += flow_wide_blocks(frames[cut++]);
            if (cut >= 1) {
                chains = 2;
                chain_b0[1] = cut;
            }
        }
    }
    if (chains > 1) {
        HIP_OK(hipEventRecord(ev_fork_, stream));
        HIP_OK(hipStreamWaitEvent(side_[0], ev_fork_, 0));
    }
    for (int step = 0; step < hp.n_flows; ++step) {
        const int i = forward ? step : hp.n_flows - 1 - step;
        const FlowLayerW& Lw = flow_[i];
        const PackedConv& post = post_of(i);
        const bool flipped = ((hp.n_flows - i) % 2) == 1;
        TensorRef x0 = sub(zp, flipped ? F / 2 : 0), x1 = sub(zp, flipped ? 0 : F / 2);
        // 16-bit modes: the whole coupling layer as ONE kernel (flow_couple16_kernel, wavenet32.hip; bit-identical to the launches below)
        if (chains > 1) {
            for (int ch = 0; ch < chains; ++ch) {
                const int b0 = chain_b0[ch], nb = chain_b0[ch + 1] - b0;
                FlowCouple16Call fc;
                fc.x0 = x0;
                fc.x0.p += (int64_t)b0 * x0.bs;
                fc.x1 = x1;
                fc.x1.p += (int64_t)b0 * x1.bs;
                fc.lens = ll + b0;
                fc.spk = spk ? spk + b0 : nullptr;
                fc.batch = nb;
                fc.tmax = 0;
                for (int b = b0; b < b0 + nb; ++b) fc.tmax = std::max(fc.tmax, frames[b]);
                fc.hidden = H;
                fc.half = F / 2;
                HIP_OK(launch_flow_couple16(Lw.pre, Lw.in_layers.data(), Lw.res_skip.data(), post, fc, arith_now_, ch == 0 ? stream : side_[0]));
            }
            continue;
        }
        if (all_fused) {
            FlowCouple16Call fc;
            fc.x0 = x0;
            fc.x1 = x1;
            fc.lens = ll;
            fc.spk = spk;
            fc.batch = B;
            fc.tmax = Lmax;
            fc.hidden = H;
            fc.half = F / 2;
            if (prof.on) {
                char full[160];
                std::snprintf(full, sizeof(full), "flow_coupling_layer|k%d|d1|C%d|e1|c%dx%d", hp.wn_k, H, F / 2, F / 2);
                double macs = (double)(F / 2) * H + (double)H * (F / 2), wbytes = (double)Lw.pre.bytes16 + (double)post.bytes16;
                for (int l = 0; l < hp.wn_layers; ++l) {
                    macs += (double)2 * H * H * hp.wn_k + (double)Lw.res_skip[l].cout * H;
                    wbytes += (double)Lw.in_layers[l].bytes16 + (double)Lw.res_skip[l].bytes16;
                }
                prof.begin(full, 2.0 * macs * (double)sum_frames, 4.0 * (double)sum_frames * (F / 2) * 3.0 + wbytes, stream, true);
            }
            HIP_OK(launch_flow_couple16(Lw.pre, Lw.in_layers.data(), Lw.res_skip.data(), post, fc, arith_now_, stream));
            prof.end(stream);
            continue;
        }
        HIP_OK(conv("flow_conv1x1", Lw.pre, mk2(x0, hout)));  // h -> hout[0,H)
        static const WaveNetLabels labels{"flow_wavenet_layer", "flow_wavenet_gated_conv", "flow_conv1x1"};
        if (run_wavenet(c, Lw.in_layers, Lw.res_skip, hp.wn_layers, labels)) return -1;
        ConvCall pc = mk2(sub(hout, H), x1);  // x1 <- x1 - (W out + b): weights negated at load (vits.cpp:506,513); forward: x1 + (W out + b)
        pc.res = x1;
        HIP_OK(conv("flow_conv1x1", post, pc));
    }
    if (chains > 1) {
        HIP_OK(hipEventRecord(ev_done_[0], side_[0]));
        HIP_OK(hipStreamWaitEvent(stream, ev_done_[0], 0));
    }
    if (o.collect_taps) {
        if (forward) snapshot("z_p", zp, F, Lmax, B, frames);
        else if (hp.n_flows % 2) snapshot_flipped("z_flow", zp, F, Lmax, B, frames);  // (odd layer count: the logical channels are the physical ones reversed)
        else snapshot("z_flow", zp, F, Lmax, B, frames);
    }
    return 0;
}

}  // namespace vits
