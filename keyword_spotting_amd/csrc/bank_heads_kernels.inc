// The two kernels of bank_heads.hip, included twice: KWS_BANK_KEYWORDS 0 -> bank_heads_kernel<H/16> and bank_heads_window_kernel<H/16, RAGGED>,
// 1 -> their keyword forms bank_keyword_heads_kernel / bank_keyword_window_kernel for a bank whose slots carry keywords of their own
// (kws_bank_set_keyword, BankSlotKeyword).  Text and not a template with a flag: the plain kernels compile the token stream they
// always had and stay the same machine code (tools/isa_diff.sh) -- as a shared force-inlined body they came out with other register
// allocations (KWS_HEAD_PROJECT, dense_heads_device.h, is a macro for the same reason).

template <int NT>
#if KWS_BANK_KEYWORDS
__global__ void __launch_bounds__(256) bank_keyword_heads_kernel(const BankKeywordHeadsParams k) {
    const BankHeadsParams& q = k.b;
#else
__global__ void __launch_bounds__(256) bank_heads_kernel(const BankHeadsParams q) {
#endif
    constexpr int H = 16 * NT;
    const DenseHeadsParams& p = q.d;
    extern __shared__ __attribute__((aligned(16))) char blds[];
    float* lgs = reinterpret_cast<float*>(blds);                                                   // [head 1 | new classes][stream][slot][8]
    int* words = reinterpret_cast<int*>(blds + kBankHeadsLogitsBytes);                             // [head][stream][slot]
    float* cols = reinterpret_cast<float*>(blds + kBankHeadsLogitsBytes + kBankHeadsWordsBytes);   // bank_stage
    float* bias = cols + (size_t)16 * H * q.bank.n_new;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, t0 = blockIdx.y * kHeadFrames, T = p.T;
    const int b = G * kStreamsPerGroup + s;
    const bool bvalid = b < p.B;
    const bool two = p.head[1].C > 0;                 // head 2 is wanted
    const int C1 = p.head[0].C, n_new = q.bank.n_new;

    if (two) bank_stage<NT>(q.bank, G * kStreamsPerGroup, p.B, cols, bias, tid);
    // A operands: Wfc^T of head 1, k-chunk kc in wa[kc]
    float wa[4 * NT];
#pragma unroll
    for (int kc = 0; kc < 4 * NT; ++kc) wa[kc] = p.head[0].wfc[kc * 64 + lane];
    const f32x4 bias4 = ld4(p.head[0].bfc + 4 * g);
    int len_s = T;
    if (p.seq_len && bvalid) len_s = p.seq_len[b];
    __syncthreads();      // the staged columns

    const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
    const int f_end = min(kBankSlots, T - t0 + 1);
    for (int f = (w == 0 && t0 == 0) ? 4 : w; f < f_end; f += 4) {      // the first block has no halo
        const int t = t0 - 1 + f;
        f32x4 v[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const float4 x = src[((size_t)t * NT + n) * 64];
            v[n] = (f32x4){x.x, x.y, x.z, x.w};
        }
        if (t >= len_s) {             // dynamic_rnn's zero row
#pragma unroll
            for (int n = 0; n < NT; ++n) v[n] = splat4(0.f);
        }
        if (p.nn_outputs && f > 0 && bvalid) {
            float4* dst = reinterpret_cast<float4*>(p.nn_outputs + ((size_t)b * T + t) * H + 4 * g);
#pragma unroll
            for (int n = 0; n < NT; ++n) dst[4 * n] = make_float4(v[n][0], v[n][1], v[n][2], v[n][3]);
        }
        KWS_HEAD_PROJECT(acc, NT, wa, bias4, v);      // dense_heads_device.h: the fused epilogue's summation order
        if (g < 2) *reinterpret_cast<f32x4*>(&lgs[((0 * 16 + s) * kBankSlots + f) * 8 + 4 * g]) = acc;
        if (two) {
            float nw[8];
            bank_project<NT>(v, cols, bias, n_new, lane, nw);
            if (g == 0) store_row8(&lgs[((1 * 16 + s) * kBankSlots + f) * 8], nw);
        }
    }
    __syncthreads();

    // one thread per (stream, slot): the rows' relu / clip, softmax and word
    for (int item = tid; item < 16 * kBankSlots; item += 256) {
        const int si = item / kBankSlots, f = item - si * kBankSlots;
        const int t = t0 - 1 + f, bi = G * kStreamsPerGroup + si;
        const bool in_call = t >= 0 && t < T;
        const int len = (p.seq_len && bi < p.B) ? p.seq_len[bi] : T;
        if (!in_call) { words[(0 * 16 + si) * kBankSlots + f] = -1; words[(1 * 16 + si) * kBankSlots + f] = -1; continue; }
        const size_t row = (size_t)bi * T + t;
        const bool out = f > 0 && bi < p.B;
        float lg[kMaxClasses], pr[kMaxClasses], raw[kMaxClasses];
        load_row8(&lgs[((0 * 16 + si) * kBankSlots + f) * 8], raw);
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) lg[c] = raw[c];
        {
            const DenseHead& hp = p.head[0];
            const int word = head_row(lg, pr, C1, p.use_relu, p.value_clip, hp.decode_thres);
            words[(0 * 16 + si) * kBankSlots + f] = t < len ? word : -1;
            if (out) {
                if (hp.logits) store_row(hp.logits + row * C1, lg, C1);
                if (hp.softmax) store_row(hp.softmax + row * C1, pr, C1);
            }
        }
        if (two) {
            const DenseHead& hp = p.head[1];
            int word = -1;
#if KWS_BANK_KEYWORDS      // the slot's own width: the C + n_used class head the user enrolled; the row's tail is zeros (bank_row, head_row)
            const int u = bank_user(q.bank, bi, p.B);
            if (u >= 0) {
                float nw[kMaxClasses];
                load_row8(&lgs[((1 * 16 + si) * kBankSlots + f) * 8], nw);
                const int n_used = k.slots[u].n_used;
                bank_row(raw, nw, C1, n_used, lg);
                word = head_row(lg, pr, C1 + n_used, p.use_relu, p.value_clip, hp.decode_thres);
            } else {
#else
            if (bank_user(q.bank, bi, p.B) >= 0) {
                float nw[kMaxClasses];
                load_row8(&lgs[((1 * 16 + si) * kBankSlots + f) * 8], nw);
                bank_row(raw, nw, C1, n_new, lg);
                word = head_row(lg, pr, hp.C, p.use_relu, p.value_clip, hp.decode_thres);
            } else {
#endif
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) { lg[c] = 0.f; pr[c] = 0.f; }
            }
            words[(1 * 16 + si) * kBankSlots + f] = t < len ? word : -1;
            if (out) {
                if (hp.logits) store_row(hp.logits + row * hp.C, lg, hp.C);
                if (hp.softmax) store_row(hp.softmax + row * hp.C, pr, hp.C);
            }
        }
    }
    __syncthreads();

    // tokens (utils/prediction.py:76-80) and the carried word
    for (int item = tid; item < 16 * kHeadFrames; item += 256) {
        const int si = item / kHeadFrames, f = 1 + (item - si * kHeadFrames);
        const int t = t0 - 1 + f, bi = G * kStreamsPerGroup + si;
        if (t >= T || bi >= p.B) continue;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            const DenseHead& hp = p.head[hd];
            if (hp.C == 0 || !hp.prev_word) continue;
            const int word = words[(hd * 16 + si) * kBankSlots + f];
            int prev;
            if (t == 0) prev = (p.reset && p.reset[bi]) ? -1 : hp.prev_in[bi];
            else prev = words[(hd * 16 + si) * kBankSlots + f - 1];
            if (hp.tokens) hp.tokens[(size_t)bi * T + t] = (int8_t)((word >= 0 && word != prev) ? word + 1 : 0);
            if (t == T - 1) hp.prev_word[bi] = word;
        }
    }
}

template <int NT, bool RAGGED>
#if KWS_BANK_KEYWORDS
__global__ void __launch_bounds__(256) bank_keyword_window_kernel(const BankKeywordWindowParams k) {
    const BankWindowParams& q = k.b;
#else
__global__ void __launch_bounds__(256) bank_heads_window_kernel(const BankWindowParams q) {
#endif
    constexpr int H = 16 * NT;
    const HeadsWindowParams& p = q.w;
    extern __shared__ __attribute__((aligned(16))) char hlds[];
    const int T = p.T, B = p.B, stride = heads_window_stride(T);
    float* lgs = reinterpret_cast<float*>(hlds);                                        // [head 1 | new classes][stream][frame of the block][8]
    int8_t* cw = reinterpret_cast<int8_t*>(hlds + kHeadsWindowLogitsBytes);             // [head][stream][stride]
    uint8_t* dl = reinterpret_cast<uint8_t*>(cw) + (size_t)2 * 16 * stride;             // [head][16 states][16 words]
    char* scratch = reinterpret_cast<char*>(dl) + 512;                                  // window 1's ring staging | window 2's
    float* cols = reinterpret_cast<float*>(scratch + window_tail_scratch_bytes(p.win[0].nq) + window_tail_scratch_bytes(p.win[1].nq));
    float* bias = cols + (size_t)16 * H * q.bank.n_new;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, b0 = G * kStreamsPerGroup;
    const int C1 = p.head[0].C, n_new = q.bank.n_new;
    window_tail_prepare(p.win[0], dl, tid);
    window_tail_prepare(p.win[1], dl + 256, tid);
#if KWS_BANK_KEYWORDS
    uint8_t* kwdl = reinterpret_cast<uint8_t*>(bias + 128);      // [16 streams][256] the slots' matchers
    int* kwn = reinterpret_cast<int*>(kwdl + 16 * 256);          // [16][n_label, n_used | own << 8]
    bank_keywords_stage(q.bank, k.slots, b0, B, p.win[1].n_label, kwdl, kwn, tid);
#endif

    if (T > 0) {
        bank_stage<NT>(q.bank, b0, B, cols, bias, tid);
        float wa[4 * NT];
#pragma unroll
        for (int kc = 0; kc < 4 * NT; ++kc) wa[kc] = p.head[0].wfc[kc * 64 + lane];
        const f32x4 bias4 = ld4(p.head[0].bfc + 4 * g);
        const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
        __syncthreads();      // the staged columns (and the label matchers)
        for (int t0 = 0; t0 < T; t0 += kHeadFrames) {
            const int f_end = min(kHeadFrames, T - t0);
            for (int f = w; f < f_end; f += 4) {
                const int t = t0 + f;
                f32x4 v[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const float4 x = src[((size_t)t * NT + n) * 64];
                    v[n] = (f32x4){x.x, x.y, x.z, x.w};
                }
                KWS_HEAD_PROJECT(acc, NT, wa, bias4, v);
                if (g < 2) *reinterpret_cast<f32x4*>(&lgs[(((0 * 16 + s) * kHeadFrames) + f) * 8 + 4 * g]) = acc;
                float nw[8];
                bank_project<NT>(v, cols, bias, n_new, lane, nw);
                if (g == 0) store_row8(&lgs[(((1 * 16 + s) * kHeadFrames) + f) * 8], nw);
            }
            __syncthreads();
            // one thread per (stream, frame): consecutive lanes on consecutive frames of one stream
            for (int item = tid; item < 16 * kHeadFrames; item += 256) {
                const int si = item / kHeadFrames, f = item - si * kHeadFrames;
                const int t = t0 + f, bi = b0 + si;
                const int Tb = RAGGED ? min(p.frames[min(bi, B - 1)], T) : T;
                if (t >= Tb) continue;
                float lg[kMaxClasses], pr[kMaxClasses], raw[kMaxClasses];
                load_row8(&lgs[(((0 * 16 + si) * kHeadFrames) + f) * 8], raw);
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) lg[c] = raw[c];
                {
                    const HeadsWindowHead& hp = p.head[0];
                    const int word = head_row(lg, pr, C1, p.use_relu, p.value_clip, hp.decode_thres);
                    cw[(0 * 16 + si) * stride + t] = (int8_t)word;
                    if (hp.softmax && bi < B) store_row(hp.softmax + ((size_t)bi * T + t) * C1, pr, C1);
                }
                {
                    const HeadsWindowHead& hp = p.head[1];
                    int word = -1;
                    if (bank_user(q.bank, bi, B) >= 0) {
                        float nw[kMaxClasses];
                        load_row8(&lgs[(((1 * 16 + si) * kHeadFrames) + f) * 8], nw);
#if KWS_BANK_KEYWORDS      // the slot's own width; the row's tail is zeros
                        const int n_used = bank_keyword_width(kwn, si);
                        bank_row(raw, nw, C1, n_used, lg);
                        word = head_row(lg, pr, C1 + n_used, p.use_relu, p.value_clip, hp.decode_thres);
#else
                        bank_row(raw, nw, C1, n_new, lg);
                        word = head_row(lg, pr, hp.C, p.use_relu, p.value_clip, hp.decode_thres);
#endif
                    } else {
#pragma unroll
                        for (int c = 0; c < kMaxClasses; ++c) pr[c] = 0.f;
                    }
                    cw[(1 * 16 + si) * stride + t] = (int8_t)word;
                    if (hp.softmax && bi < B) store_row(hp.softmax + ((size_t)bi * T + t) * hp.C, pr, hp.C);
                }
            }
            __syncthreads();      // the block's logits are consumed, and (last block) the chunk's words are complete
        }
    } else {
        __syncthreads();          // the label matchers
    }

    // ---- the two windows, then the coupling (heads_window_kernel's, unchanged)
    WindowTailRegs<4> req1, req2;
    window_tail_request<4>(p.win[0], B, b0, tid, req1);
    window_tail_request<4>(p.win[1], B, b0, tid, req2);
    const int bt = min(b0 + (tid >> 4), B - 1);                  // window_tail's stream of this lane
    const int Tt = RAGGED ? min(p.frames[bt], T) : T;
    const bool live = RAGGED ? p.skip[bt] == 0 : true;
    const bool hit1 = window_tail<4>(p.win[0], B, b0, Tt, cw, stride, dl, scratch, tid, req1, live);
#if KWS_BANK_KEYWORDS      // window 2 walks the matcher of the lane's stream's slot; window 2's own where the slot has none
    const int ts = tid >> 4;
    const uint8_t* dl2 = (kwn[2 * ts + 1] & 256) ? kwdl + ts * 256 : dl + 256;
    const bool hit2w = window_tail<4, true>(p.win[1], B, b0, Tt, cw + 16 * stride, stride, dl2, scratch + window_tail_scratch_bytes(p.win[0].nq),
                                            tid, req2, live, kwn[2 * ts]);
#else
    const bool hit2w = window_tail<4>(p.win[1], B, b0, Tt, cw + 16 * stride, stride, dl + 256, scratch + window_tail_scratch_bytes(p.win[0].nq),
                                      tid, req2, live);
#endif
    if ((tid & 15) == 0 && b0 + (tid >> 4) < B) {
        if (live) {
            // a stream without a slot never reports head 2 (its window holds wordless entries only; this covers the empty label too)
            const bool hit2 = hit2w && bank_user(q.bank, bt, B) >= 0;
            const bool fired = hit1 || hit2;
            if (fired) {                                         // detector.py:202-208, whichever head fired
                p.win[0].head[bt] = 0; p.win[0].count[bt] = 0;
                p.win[1].head[bt] = 0; p.win[1].count[bt] = 0;
            }
            if (p.restart) p.restart[bt] = fired ? 1 : 0;
            p.hit[bt] = (hit1 ? 1 : 0) | (hit2 ? 2 : 0);
        } else {
            p.hit[bt] = 0;
        }
    }
}
