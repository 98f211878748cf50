/* kws_amd.h -- C ABI of the MI355X-native streaming GRU keyword-spotting path.
 *
 * Drop-in boundary.  Every entry point replaces one interface of the reference
 * (paths relative to colinsongf/keyword_spotting):
 *
 *   kws_create / kws_destroy   tf.import_graph_def + tf.Session on the frozen DeployModel graph
 *                              (detector.py:134-146; export list main.py:339-342)
 *   kws_step                   sess.run(['model/softmax:0','model/logit:0','model/rnn_states:0'],
 *                              {'model/inputX:0', 'model/rnn_initial_states:0'})
 *                              (detector.py:190-193, :220-223, :280-283) on the mel-input variant
 *                              of the graph (models/rnn_ctc.py:150-153), batched over B streams;
 *                              arithmetic of models/rnn_ctc.py:155-165,202-284
 *   kws_ctc_decode             utils/prediction.py:18 ctc_decode, :65 ctc_decode2, :89 ctc_decode_strict
 *   kws_ctc_predict            utils/prediction.py:111 ctc_predict
 *   kws_vad                    utils/basic_vad.py:17 vad
 *   kws_stream_feed            one iteration of HotwordDetector.start's loop, detector.py:158-209, for B streams
 *   kws_stream_create_heads    ... on a customised-keyword model: both dense layers decoded per chunk ("do softmax and decode
 *                              respectively", README "Customize keyword"), the decisions ORed (server_demo.py:122-129)
 *   kws_enroll_fit             the training of the README's "Customize keyword" step: tf.nn.ctc_loss + AdamOptimizer on the new
 *                              columns of the class projection (models/rnn_ctc.py:59-101), frozen stack
 *   kws_ctc_beam_search        tf.nn.ctc_beam_search_decoder as models/rnn_ctc.py:105-110, :166-176 would call it (commented out
 *                              there): top paths and their log-probabilities
 *   kws_ctc_align              the "alignment for word" the README's frame-wise experiment (README.md:48,72) took from an outside
 *                              model that "can only label the peak frame of each word": word spans, best path, posteriors
 *   kws_octbit_matmul          REGISTER_OP("OctbitMatMul") octbit/octbit_ops_reg.cc:7-15,
 *                              OctbitMatMulOp::Compute octbit/octbit_mat_mul_op.cc:49-183
 *   kws_octbit_quantize        octize_weight_int8_signed octbit/octbit_graph.py:191-215
 *
 * Conventions
 *   - plain C types only; every tensor pointer is CALLER-OWNED DEVICE memory (hipMalloc / a PyTorch
 *     tensor's data_ptr) unless the parameter is documented as host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All work is
 *     enqueued asynchronously on it; no entry point synchronises the device except the create / destroy calls,
 *     kws_kernel_times, kws_reserve, the first kws_window_step of a window (allocates its frame ring) -- and kws_step only
 *     when the call needs more scratch than kws_reserve or any earlier call provided (it then grows the handle's scratch
 *     block, which waits for the device once; kws_scratch_stats counts those events).
 *   - return value: KWS_OK or a negative kws_status.  No exceptions, no abort.  The message for the
 *     last failure on the calling thread is kws_last_error().
 *   - a handle is immutable after kws_create except for its scratch buffer and profiling slots: ONE host thread at a
 *     time per handle.  The reference's OctbitMatMulOp::Compute is re-entrant (octbit/octbit_mat_mul_op.cc:49) because it
 *     allocates its temporaries per call; here the inter-layer seams belong to the handle, so the unit of concurrency is the
 *     handle (0.64 MB of weights + scratch each): one per host thread, each on its own HIP stream -- different handles are
 *     fully independent (tests/test_gpu_soak.py drives two threads on two handles).  Sharing one handle is detected, not
 *     undefined: a thread that enters kws_step / kws_reserve / kws_kernel_times while another is inside gets KWS_ERR_BUSY
 *     and nothing is launched; calls that are serialised by the caller but arrive on a different stream than the call before
 *     are ordered behind it ON THE DEVICE (every call records an event at its end, the next call's stream waits for it when it
 *     is another stream): no host wait, nothing that touches other handles' work, legal under stream capture.  (Streams are
 *     told apart by their handle value: do not destroy a stream with this handle's work still queued and expect a new stream
 *     that reuses the address to be ordered behind it.)  kws_stream_feed holds its MODEL handle for the whole iteration: stream
 *     managers that are fed concurrently need a model handle each; any number of them may share one handle when fed in turn.
 */
#ifndef KWS_AMD_H_
#define KWS_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum kws_status {
    KWS_OK = 0,
    KWS_ERR_INVALID_ARGUMENT = -1, /* the TF InvalidArgumentError cases: bad dims, null ptr, K%64 ... */
    KWS_ERR_UNSUPPORTED = -2,      /* shape outside what the kernels are built for                    */
    KWS_ERR_HIP = -3,              /* a HIP runtime call failed (message has hipGetErrorString)       */
    KWS_ERR_NO_DEVICE = -4,        /* no gfx950 device visible                                        */
    KWS_ERR_OUT_OF_MEMORY = -5,
    KWS_ERR_BUSY = -6              /* another host thread is inside kws_step / kws_reserve / kws_kernel_times / kws_stream_feed on this handle */
} kws_status;

/* Model shape: config/rnn_config.py:57-99 (n_mel :63, hidden_size :84, num_layers :76,
 * num_classes :88-91, use_relu :83, value_clip :80). */
typedef struct kws_config {
    int32_t n_mel;       /* I : mel bins per 10 ms frame                                   */
    int32_t hidden;      /* H : GRU units per layer; supported: 64, 128, 256                */
    int32_t num_layers;  /* L : 1..8                                                        */
    int32_t num_classes; /* C : 3..8 (space, words..., blank)                               */
    int32_t use_relu;    /* models/rnn_ctc.py:280                                           */
    float value_clip;    /* models/rnn_ctc.py:282 : >0 and use_relu -> clip logits to [0,20] */
    int32_t precision;   /* KWS_FP32 (reference arithmetic); KWS_BF16 (BASELINE configs[2]: bf16 weights and
                            matmul inputs, fp32 accumulate / state / activations; H=128, L<=2, n_mel%4==0, <=64);
                            KWS_INT8 (BASELINE configs[2], the graph octbit/octbit_graph.py:461-485 produces: the
                            gate/candidate MatMuls of cell_1.. and the class projection are OctbitMatMul calls --
                            name rule :218-225, weights quantised at kws_create by :191-215, op arithmetic
                            octbit_mat_mul_op.cc:90-181 incl. the int16 pair saturation, activation range per
                            stream as the batch-1 graph has it; layer 0, biases, activations fp32; H=128) */
} kws_config;
enum { KWS_FP32 = 0, KWS_BF16 = 1, KWS_INT8 = 2,
       /* fp32 results on the fp16 matrix pipe: every matmul operand split into two fp16 pieces (22 mantissa bits), three
          v_mfma_f32_16x16x32_f16 per product, fp32 accumulation, activations and state (csrc/gru_f16x3.hip).  Meets the
          fp32 path's tolerance (logits within 1e-4 of the reference semantics; observed ~3e-6) at ~2.5x its throughput;
          it is NOT bit-identical to KWS_FP32.  Every matrix weight must be finite with |w| < 64 (else KWS_ERR_UNSUPPORTED naming it).
          GRU handles (kws_create): hidden 128 on the register-resident kernels (n_mel % 4 == 0 and <= 64), otherwise the
          L2-streaming ones (csrc/gru_f16x3_generic.hip); any num_layers.  Attention handles (kws_attention_create_precision): the
          whole config space kws_attention_create takes; the embedding, qkv and FFN products run split (csrc/attention_f16x3.hip),
          the attention core, layer norm and output projection stay fp32. */
       KWS_F16X3 = 3 };

typedef struct kws_model* kws_handle;

enum { KWS_KERNEL_AUTO = 0, KWS_KERNEL_GENERIC = 1, KWS_KERNEL_RESIDENT = 2 };
enum { KWS_DECODE = 0, KWS_DECODE2 = 1, KWS_DECODE_STRICT = 2 };

/* "kws_amd <ver> (gfx950; HIP x.y.z; <compiler version>; bf16 mfma-vgpr-form=<0|1>; f16x3 mfma-vgpr-form=<0|1>)": the compiler
 * is part of the version because the kernels depend on hand-placed MFMA hazard fences and, for the two files named, on an
 * internal LLVM option that csrc/Makefile applies only when this hipcc accepts it. */
const char* kws_version(void);
/* sizeof(kws_config) / sizeof(kws_frontend_config) as this library was compiled: a binding written in another
 * language (ctypes, cffi, JNI ...) compares it with its own struct declaration at load time, so a field added here
 * can never be read past the end of a caller's shorter struct. */
size_t kws_sizeof_config(void);
size_t kws_sizeof_frontend_config(void);
/* Message of the last error raised on this thread ("" if none). */
const char* kws_last_error(void);

/* Bytes of the canonical fp32 weight blob for `cfg`:
 *   per layer l (I_0 = n_mel, I_l = hidden):  Wg[I_l+H, 2H]  bg[2H]  Wc[I_l+H, H]  bc[H]
 *   then Wfc[H, C]  bfc[C]           -- TF variable layouts, row-major, gate order [r, u]. */
size_t kws_weights_nbytes(const kws_config* cfg);

/* Stages the weights on the current HIP device (re-tiled into MFMA fragment order) and returns a
 * handle.  `weights_blob` is HOST memory of kws_weights_nbytes(cfg) bytes. */
int kws_create(const kws_config* cfg, const void* weights_blob, size_t nbytes, kws_handle* out);
/* Cell wrappers of the reference's get_cell (models/rnn_ctc.py:179-199; config/rnn_config.py:78-79 use_residual /
 * use_layer_norm, both off by default): every layer is ResidualWrapper(LayerNormalizer(GRUCell)), the residual on layers >= 1
 * only (utils/custom_wrapper.py:95-158).  Each field is 0 or 1.
 *   use_layer_norm  the layer's input x (width I_l; layer 0: the mel frame) is normalised per stream and frame before the cell:
 *                   x^ = (x - mean(x)) / sqrt(var(x) + 1e-5) * ibeta + igamma, with the population variance around the mean.
 *                   The reference's names are swapped (_ln(inputs, ibeta, igamma) binds to _ln(input, s, b)): ibeta is the
 *                   SCALAR SCALE (shape [], TF initialises it to 0), igamma the PER-FEATURE SHIFT (shape [I_l], initialised to 1).
 *   use_residual    the output of layer l >= 1 is 0.7071067811865475 (h' + x), x the layer's input before the layer norm; the
 *                   next layer and the dense layer read that, the recurrent state (state_out, model/rnn_states:0) stays h'.
 *                   Rows past seq_len still emit the zero row (logits = bfc) and keep the state.  No effect with num_layers = 1.
 * kws_weights_nbytes_wrapped: the canonical blob, followed -- with use_layer_norm -- by each layer's ibeta (1 float) and igamma
 * (I_l floats), in layer order; the residual adds nothing.  kws_create_wrapped takes that blob.  A NULL or all-zero `wrap` is
 * kws_weights_nbytes / kws_create exactly.  Wrapped handles run the fp32 generic kernels only (KWS_FP32; any other precision:
 * KWS_ERR_UNSUPPORTED): KWS_KERNEL_AUTO picks them, KWS_KERNEL_RESIDENT is refused (KWS_ERR_UNSUPPORTED), and a stream manager
 * on such a handle runs its decode window as a launch of its own (window_inc_kernel) behind the GRU layers.  kws_selftest on a
 * wrapped handle runs the random case only (the published TensorFlow constants are for the plain cell), with both wrappers in
 * the host loop and random ibeta / igamma. */
typedef struct kws_cell_wrappers {
    int32_t use_layer_norm;
    int32_t use_residual;
} kws_cell_wrappers;
size_t kws_sizeof_cell_wrappers(void);
size_t kws_weights_nbytes_wrapped(const kws_config* cfg, const kws_cell_wrappers* wrap);   /* 0: invalid config or wrappers */
int kws_create_wrapped(const kws_config* cfg, const kws_cell_wrappers* wrap, const void* weights_blob, size_t nbytes,
                       kws_handle* out);
/* Releases the handle and always returns KWS_OK (the handle is gone afterwards, whatever it reports: never retry).  An
 * error a finished asynchronous step had raised and nobody collected is left in kws_last_error(); call kws_poll_error
 * first to get it as a status.  Stream handles created on it (kws_stream_create) fail cleanly afterwards. */
int kws_destroy(kws_handle h);

/* Kernel family used by kws_step (fp32): AUTO picks the register-resident kernels when the shape allows
 * (hidden == 128 and n_mel in {32, 40, 48, 60, 64}) and the handle has no cell wrappers, else the generic ones (hidden
 * 64/128/256, any n_mel).  RESIDENT on an unsupported shape or a wrapped handle -> KWS_ERR_UNSUPPORTED.  Ignored by the bf16 stack. */
int kws_set_kernel(kws_handle h, int kind);
/* Pre-sizes the handle's scratch for calls of B streams x up to T frames: afterwards kws_step with this B and T' <= T
 * never allocates or synchronises, whichever launch layout it picks for that shape (sequential layers, layers overlapped
 * on HIP streams, layer-pipelined launch).  A later call with a DIFFERENT B may select a layout this call did not size
 * (e.g. a smaller batch that becomes eligible for the layer-pipelined launch) and then grows the scratch once, which
 * synchronises: reserve every batch size you will use.  The scratch only grows. */
int kws_reserve(kws_handle h, int B, int T);
/* bytes_reserved: device scratch currently held for inter-layer seams; allocations: how many times it (or another
 * batch-sized side buffer) was (re)allocated -- each of those synchronised the device.  Either pointer may be NULL. */
int kws_scratch_stats(kws_handle h, size_t* bytes_reserved, int32_t* allocations);
/* KWS_OK, or the error a finished asynchronous step of this handle raised on the device (today: a layer-pipelined
 * launch whose wait for the layer below timed out -- the results of that step are invalid).  Does not synchronise: to
 * validate a given step, synchronise its stream first.  The same condition is also reported by the next kws_step and
 * by kws_kernel_times, whichever comes first; reporting clears it.  (kws_destroy only leaves it in kws_last_error().) */
int kws_poll_error(kws_handle h);

/* Proves the kernels `h` would launch (its shape and precision; for fp32 both the register-resident and the generic
 * family where the shape allows) against known answers the library carries itself: TensorFlow's published GRUCell /
 * MultiRNNCell unit-test constants (0.175991, 0.156736, 0.13248) embedded in the handle's shape, and 19 streams x 8
 * random frames against a plain double-precision host loop of the cell (models/rnn_ctc.py:179-185,228-243 semantics).
 * On a handle with cell wrappers (kws_create_wrapped) the TensorFlow constants are skipped -- they hold for the plain cell
 * only -- and the random case runs the wrapped kernels against the host loop with both wrappers, random ibeta and igamma.
 * Uses temporary handles and buffers, synchronises the device, a few milliseconds.  KWS_OK, or KWS_ERR_HIP with a
 * message naming the kernel, the deviation and kws_version().  With KWS_SELFTEST=1 in the environment every
 * kws_create runs it and fails the same way.  (There is still no CPU fallback: a failed self-test is an error.) */
int kws_selftest(kws_handle h);
/* Name of the kernel(s) the last kws_step of this handle launched for profiling slot `slot` (0..L-1; "" when that layer
 * ran inside another slot's launch), e.g. "gru_layer_resident<32, false, true>".  buf: host memory of n bytes. */
int kws_last_launch(kws_handle h, int slot, char* buf, size_t n);

/* Advances B independent streams by T frames (one 10 ms hop each).
 *   mel        [B,T,I]  f32, 16-byte aligned         model/inputX:0 (mel variant), batch-major
 *   state_in   [L,B,H]  f32                          model/rnn_initial_states:0
 *   logits     [B,T,C]  f32   out, may be NULL       model/logit:0
 *   softmax    [B,T,C]  f32   out, may be NULL       model/softmax:0
 *   state_out  [L,B,H]  f32   out, may alias state_in  model/rnn_states:0
 *   seq_len    [B] i32, may be NULL (= T): rows with t >= seq_len[b] keep their state and emit the
 *              zero-output row (logits = bfc), as dynamic_rnn(sequence_length=...) does
 *   reset_mask [B] u8,  may be NULL: non-zero -> stream b starts this call from the zero state and
 *              prev_word = -1 (detector.py:313-316 clean_state + prob_queue.clear())
 *   tokens     [B,T] i8 out, may be NULL: fused ctc_decode2 -- 0, or the word (1..C-2) emitted at
 *              frame t (utils/prediction.py:74-80 with thres = decode2_thres)
 *   prev_word  [B] i32 in/out, required iff tokens != NULL: ctc_decode2's pre_word carried across
 *              calls (-1 = none)
 * T == 0 or B == 0 is a no-op (state_out = state_in). */
int kws_step(kws_handle h, const float* mel, const float* state_in, float* logits, float* softmax,
             float* state_out, const int32_t* seq_len, const uint8_t* reset_mask, int8_t* tokens,
             int32_t* prev_word, float decode2_thres, int B, int T, void* stream);

/* Customised-keyword models (the reference's README.md:109-132 and server_demo.py:107-129): the GRU stack is frozen, a second
 * projection [H, C2] is trained beside the first, and the model is served with both dense layers on the same top-layer rows
 * (model/softmax1:0, model/softmax2:0), next to those rows themselves (model/nn_outputs:0).
 *   kws_weights_nbytes_heads  the canonical blob of `cfg`, then Wfc2[H, C2] and bfc2[C2]; 0: invalid config, C2 outside 3..8,
 *                             or a precision the heads do not serve.
 *   kws_create_heads          a model handle with the second head.  KWS_FP32 only: bf16 (no seam between its layers), int8 and
 *                             f16x3 (seams in another format) are KWS_ERR_UNSUPPORTED, decided before the device is probed;
 *                             there is no wrapped form.  The handle is a normal model handle: kws_step, kws_stream_create,
 *                             kws_selftest and the rest behave as on a kws_create handle of the canonical part of the blob
 *                             (head 1, fused into the last layer's launch); kws_selftest additionally proves kws_step_heads.
 *   kws_step_heads            kws_step with both heads: every layer writes its rows to a seam (one launch per layer, the
 *                             kernel family of kws_set_kernel; never the overlapped or layer-pipelined layouts) and one more
 *                             launch reads the top layer's seam once for everything below.  mel, state_in, state_out, seq_len,
 *                             reset_mask, B, T, stream: as kws_step.  head1 / head2 (either may be NULL: that head is not
 *                             computed) carry, per head, what kws_step takes for its one: logits [B,T,C_i], softmax [B,T,C_i],
 *                             tokens [B,T] (each may be NULL), prev_word [B] in/out (required iff tokens != NULL) and the
 *                             head's own decode2_thres.  reset_mask sets both heads' prev_word to -1.
 *                             nn_outputs [B,T,H] f32, 16-byte aligned, may be NULL: the top layer's output rows, batch-major
 *                             (dynamic_rnn's outputs, models/rnn_ctc.py:238-243).
 *                             Rows with t >= seq_len[b]: nn_outputs = 0, logits = bfc_i (then relu / clip), tokens = 0, and
 *                             the frame counts as "no word" for the token rule and for prev_word.
 *                             Only on a kws_create_heads handle (else KWS_ERR_INVALID_ARGUMENT).  kws_reserve on such a
 *                             handle sizes the scratch for kws_step and kws_step_heads alike.  With profiling on, the heads'
 *                             launch is timed in slot L-1 with the top layer, and kws_last_launch names both kernels. */
typedef struct kws_head_io {
    float* logits;
    float* softmax;
    int8_t* tokens;
    int32_t* prev_word;
    float decode2_thres;
} kws_head_io;
size_t kws_sizeof_head_io(void);
size_t kws_weights_nbytes_heads(const kws_config* cfg, int32_t num_classes2);
int kws_create_heads(const kws_config* cfg, int32_t num_classes2, const void* weights_blob, size_t nbytes, kws_handle* out);
int kws_step_heads(kws_handle h, const float* mel, const float* state_in, float* state_out, const int32_t* seq_len,
                   const uint8_t* reset_mask, float* nn_outputs, const kws_head_io* head1, const kws_head_io* head2, int B, int T,
                   void* stream);

/* Per-kernel timing (bench.py roofline): when enabled, kws_step brackets each kernel launch with
 * hipEvents on `stream`.  kws_kernel_times synchronises those events and returns, per layer kernel
 * slot (0..L-1), the summed milliseconds and the launch count since the last reset. */
int kws_set_profiling(kws_handle h, int enable);
int kws_kernel_times(kws_handle h, float* ms_sum /*[L]*/, int32_t* launches /*[L]*/, int reset);

/* Greedy CTC collapse over whole windows, one GPU thread per stream.
 *   kind      KWS_DECODE (uses lockout, thres, loose_thres; columns 1:5 -> needs C >= 5),
 *             KWS_DECODE2 (thres), KWS_DECODE_STRICT (lockout, thres)
 *   softmax   [B,T,C] f32;  lengths [B] i32 or NULL (= T)
 *   words     [B,max_words] i32 out: emitted words in order (without the interleaved zeros of the
 *             reference's [0,w,0,...] format);  counts [B] i32 out (may exceed max_words: truncated) */
int kws_ctc_decode(int kind, const float* softmax, const int32_t* lengths, int B, int T, int C,
                   int lockout, float thres, float loose_thres, int32_t* words, int32_t* counts,
                   int max_words, void* stream);

/* ctc_predict: hit[b] = 1 iff the digits of label (host string of '1'..'9') occur contiguously in
 * words[b, :min(counts[b], max_words)]. */
int kws_ctc_predict(const int32_t* words, const int32_t* counts, int B, int max_words,
                    const char* label, int32_t* hit, void* stream);

/* vad: speech[b] = (sum_n |pcm[b,n]| > thres).  pcm [B,N] f32. */
int kws_vad(const float* pcm, int B, int N, float thres, uint8_t* speech, float* abs_sum_or_null,
            void* stream);

/* PCM -> mel front-end of the deploy graph (models/rnn_ctc.py:134-149, utils/stft.py:27-81): frames of
 * fft_size samples every hop_size (no padding, no window), |rfft|, projection on librosa.filters.mel(sr, n_fft,
 * n_mels, fmin, fmax) (Slaney scale, area-normalised).  pcm [B,N] f32 -> mel [B,T,n_mel], T = 1+(N-fft)/hop
 * (kws_frontend_frames).  fft_size must be a multiple of 16. */
typedef struct kws_frontend_config {
    int32_t samplerate, fft_size, hop_size, n_mel;
    float fmin, fmax;
} kws_frontend_config;
typedef struct kws_frontend* kws_frontend_handle;
int kws_frontend_create(const kws_frontend_config* cfg, kws_frontend_handle* out);
int kws_frontend_destroy(kws_frontend_handle h);
int kws_frontend_frames(const kws_frontend_config* cfg, int n_samples);
int kws_frontend_run(kws_frontend_handle h, const float* pcm, int B, int n_samples, float* mel, void* stream);
/* The streaming form (detector.py:179-183): the signal of stream b is carry[b] followed by chunk[b] --
 * np.concatenate((self.res, data)) -- read in place, never materialised; mel [B,T,n_mel] with
 * T = kws_frontend_frames(n_carry + n_chunk) (nothing is written when that is 0).  Also writes next_carry [B,n_next],
 * the last n_next samples of that signal (self.res = data[-res:]); it must not overlap carry or chunk. */
int kws_frontend_run_carry(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk,
                           int B, float* mel, float* next_carry, int n_next, void* stream);
/* Copies the fp32 mel basis [n_mel, fft/2+1] (host memory) the handle was built with -- for inspection/tests. */
int kws_frontend_mel_basis(kws_frontend_handle h, float* basis_host);

/* Feature front-ends behind the same handle type: what the reference's graphs and reader build from the un-windowed STFT.
 *   KWS_FEAT_MEL, power 1   |rfft| -> mel: kws_frontend_create(cfg) is exactly {cfg, KWS_FEAT_MEL, 1, 0}
 *   KWS_FEAT_MEL, power 2   |rfft|^2 -> mel (reader.py:267-268)
 *   KWS_FEAT_MFCC           config.mfcc (utils/mfcc.py:20-99; models/attention_ctc.py:249-250), per utterance of T frames:
 *                             m = |rfft|^2 . mel_basis^T      squared whatever config.power says (:77); base.n_mel filters
 *                             S = 10 log10(max(1e-10, m))     ref_value 1, and NO top_db: every call site leaves it None
 *                             c = S . D                       D = the orthonormal DCT-II basis [n_mel, n_mfcc] in float32 (:33-42,:93)
 *                             d[t] = c[min(t+1, T-1)] - c[max(t-1, 0)]     (_delta_order shifts by one frame whatever its order)
 *                             row t = [c | d / 2 | 0.3 d]     3 * n_mfcc features (:96-99); T = 1 gives zero deltas
 * kws_frontend_feature_size is the row width: n_mel, or 3 * n_mfcc.  The deltas' right-hand edge makes MFCC a transform of a
 * WHOLE utterance: kws_frontend_run_carry and kws_stream_create refuse every handle that is not (KWS_FEAT_MEL, power 1) with
 * KWS_ERR_UNSUPPORTED.  MFCC and power 2 exist for fft_size = 400 only (the FFT kernel; KWS_ERR_UNSUPPORTED otherwise, naming
 * the field); n_mfcc outside 1..min(n_mel, 32) or power outside {1, 2} is KWS_ERR_INVALID_ARGUMENT.
 *
 * kws_frontend_run_lengths: B utterances in rows of n_max samples, utterance b with n_b = clamp(n_samples[b], 0, n_max) of them
 * (n_samples == NULL: n_max for all).  out is [B, T_max, feature_size] with T_max = kws_frontend_frames(n_max); utterance b has
 * T_b = kws_frontend_frames(n_b) rows, rows t >= T_b are written as 0, and samples at or past n_b are never read into a result
 * (the padding may hold anything).  The delta edges of utterance b are its own T_b.  One launch for mel output, two for MFCC
 * (the coefficients, then the deltas in place), whatever B; no host work per utterance, no allocation, no device-wide wait, any
 * stream.  kws_frontend_run on an MFCC or power-2 handle is kws_frontend_run_lengths with n_samples == NULL.  On a
 * (KWS_FEAT_MEL, power 1) handle with another fft_size than 400 only n_samples == NULL is supported. */
enum { KWS_FEAT_MEL = 0, KWS_FEAT_MFCC = 1 };
typedef struct kws_feature_config {
    kws_frontend_config base;   /* samplerate, fft_size, hop_size, n_mel (= mel filters), fmin, fmax */
    int32_t kind;               /* KWS_FEAT_MEL | KWS_FEAT_MFCC */
    int32_t power;              /* KWS_FEAT_MEL only: 1 (|X|) or 2 (|X|^2); MFCC ignores it */
    int32_t n_mfcc;             /* KWS_FEAT_MFCC: 1..min(n_mel, 32); KWS_FEAT_MEL ignores it */
} kws_feature_config;
size_t kws_sizeof_feature_config(void);
int kws_frontend_create_features(const kws_feature_config* cfg, kws_frontend_handle* out);
int kws_frontend_feature_size(kws_frontend_handle h);
int kws_frontend_run_lengths(kws_frontend_handle h, const float* pcm /*[B, n_max] device*/, const int32_t* n_samples /*[B] device or NULL*/,
                             int B, int n_max, float* out /*[B, T_max, feature_size] device*/, void* stream);
/* Copies the fp32 DCT basis [n_mel, n_mfcc] (host memory) of an MFCC handle -- for inspection/tests. */
int kws_frontend_dct_basis(kws_frontend_handle h, float* basis_host);

/* The features the reference's models are trained and validated on (process_wav.py:38-44,69-78 -> reader.py:264-269; the same
 * framing in server_demo.py:59-82): |librosa.stft(y, 400, 160)| instead of the deploy graph's un-windowed, un-padded frames, in
 * front of the same kws_feature_config.  For one utterance x[0..n) of float32 samples, h = hop_size, c = pre_emphasis:
 *   y[0] = x[0], y[i] = x[i] - fl32(c * x[i-1])     only if c != 0 (config.pre_emphasis: 0.97); float32, multiply and subtract
 *                                                   rounded separately, as numpy does it
 *   T(n) = 1 + n / h for n >= 201, 0 for n <= 200   center=True: frame t is centred on sample h t
 *   frame t, tap i in [0, 400): s = h t + i - 200; s < 0: s = -s; s >= n: s = 2 (n - 1) - s; frame[i] = y[s] * w[i]
 *                                                   np.pad(y, 200, mode='reflect'): one reflection at most for n >= 201
 *   w[i] = 0.5 - 0.5 cos(2 pi i / 400)              the periodic Hann window (scipy.signal.get_window('hann', 400)), float32
 *   |rfft(frame, 400)| -> what cfg.feat says: mel of |X| or |X|^2, or MFCC + deltas with the delta edges at T(n_b)
 * np.pad's REPEATED reflection of a signal shorter than the pad (n <= 200) is deliberately not reproduced: such an utterance has no
 * frames.  fft_size = 400 and the FFT kernel only (KWS_ERR_UNSUPPORTED otherwise, naming the field; KWS_FRONTEND_DENSE=1 included).
 * {feat, KWS_FRAMES_DEPLOY, 0} is kws_frontend_create_features(&feat) exactly; KWS_FRAMES_DEPLOY with pre_emphasis != 0, a framing
 * outside the enum, or a pre_emphasis that is not finite or outside [0, 1) is KWS_ERR_INVALID_ARGUMENT.
 * A dataset handle runs through kws_frontend_run_lengths (kws_frontend_run forwards to it): out is [B, T(n_max), feature_size],
 * rows t >= T(n_b) are written as 0, samples at or past n_b are never read into a result (the reflection reads indices < n_b
 * only); one launch for mel output, two for MFCC.  Centred frames need the utterance's end: kws_frontend_run_carry and
 * kws_stream_create (so every stream feed) refuse a dataset handle with KWS_ERR_UNSUPPORTED.
 * kws_frontend_frames_of is the handle's own frame count of n_samples -- the deploy rule (kws_frontend_frames, which keeps its
 * meaning) or T(n) above.  kws_frontend_window copies the 400 float32 window values (host memory) of a dataset handle. */
enum { KWS_FRAMES_DEPLOY = 0, KWS_FRAMES_DATASET = 1 };
typedef struct kws_dataset_config {
    kws_feature_config feat;
    int32_t framing;            /* KWS_FRAMES_DEPLOY | KWS_FRAMES_DATASET */
    float pre_emphasis;         /* KWS_FRAMES_DATASET only: 0 (none) or the coefficient, in [0, 1) */
} kws_dataset_config;
size_t kws_sizeof_dataset_config(void);
int kws_frontend_create_dataset(const kws_dataset_config* cfg, kws_frontend_handle* out);
int kws_frontend_frames_of(kws_frontend_handle h, int n_samples);
int kws_frontend_window(kws_frontend_handle h, float* window_host);

/* The training reader's noise augmentation (reader.py:207-280, config/rnn_config.py:67-73): a slice of a background-noise
 * spectrogram is added to the utterance's |STFT| -- in the LINEAR domain, before the squaring and the mel / MFCC projection -- at a
 * level of gain_db relative to the utterance's own (compute_db, reader.py:325-332).  Two entry points, fft_size = 400 and the FFT
 * kernel only (KWS_ERR_UNSUPPORTED otherwise), on every handle that kws_frontend_run_lengths serves: either framing, with and
 * without pre-emphasis, whatever the handle's features are.
 *
 * kws_frontend_linear_size: 201, the bins 0..200 of a row of the linear spectrum.
 * kws_frontend_run_linear: kws_frontend_run_lengths with the magnitudes themselves as the output.  B utterances in rows of n_max
 *   samples, n_b = clamp(n_samples[b], 0, n_max) of them in utterance b (NULL: n_max for all) ->
 *     spec [B, T_max, 201]    |X| of the handle's frames, T_max = kws_frontend_frames_of(n_max) >= 1; rows t >= T_b are written as 0
 *     frames_out [B] int32    T_b = kws_frontend_frames_of(n_b)
 *     energy_out [B]          sum over t < T_b and the 201 bins of spec^2: what compute_db sums (the zero rows add nothing).  A
 *                             frame's bins are summed in float32 in one fixed order, the frames of an utterance in float64 in one
 *                             fixed order, rounded once: the value does not depend on what else is in the batch.
 *   Two launches (the spectra, then one workgroup per utterance for the energies), no allocation, any stream.  Noise clips are
 *   utterances and take the same call.
 * kws_frontend_augment: R rows of the handle's own features from a set of clean spectra (spec [B, T_max, 201], frames [B],
 *   energy [B]: what kws_frontend_run_linear wrote) and a set of noise spectra (the same triple, [K, Tn_max, 201]).  Row r, with
 *   b = src[r], k = noise[r], T_r = frames[b]:
 *     db(E, n) = 10 log10(E / fft_size^2 / n)
 *     factor   = 10 ^ ((db(energy[b], frames[b]) - db(noise_energy[k], noise_frames[k]) + gain_db[r]) / 20)
 *              = sqrt((energy[b] / frames[b]) / (noise_energy[k] / noise_frames[k])) * 10 ^ (gain_db[r] / 20), evaluated in double
 *     mixed[t, f] = spec[b, t, f] + factor * noise_spec[k, start[r] + t, f]      t < T_r; a noise frame at or past noise_frames[k]
 *                                                                             adds 0 (the reader's zero padding of its noise)
 *     out[r, t, :] = the handle's features of mixed[t, :] -- mel of mixed, mel of mixed^2, or MFCC + deltas of mixed^2 with the delta
 *                    edges at T_r; rows t >= T_r are written as 0.  out is [R, T_max, feature_size].
 *   All arrays are DEVICE memory, which the host cannot check: the kernels decide the edge cases, and read nothing out of bounds in
 *   any of them.
 *     noise[r] outside [0, K)                         no noise for that row (-1 by convention)
 *     src[r] outside [0, B)                           a row of zeros
 *     start[r] < 0                                    read as 0
 *     frames[b] / noise_frames[k]                     clamped to [0, T_max] / [0, Tn_max]
 *     energy[b] == 0 (or not positive: NaN)           factor = 0 (the reference's 10 ** -inf)
 *     noise_energy[k] not positive, noise_frames[k] == 0, or a factor that is not finite (gain_db)
 *                                                     factor = 0, no noise (the reference would produce NaN)
 *   A row without noise holds exactly the bits kws_frontend_run_lengths gives a (KWS_FEAT_MEL, power 1) handle; on power 2 and
 *   MFCC it differs in the last bits, because this path squares the magnitude (reader.py:267-268) where that one takes re^2 + im^2.
 *   A row's bits do not depend on the other rows of the call.  One small launch that turns the row arrays into a plan, the feature
 *   launch and, for MFCC, the delta launch; the plan (36 bytes per row) is a stream-ordered allocation released behind them.
 * B, n_max, K, Tn_max, R, T_max < 1 and null pointers are KWS_ERR_INVALID_ARGUMENT, decided before the device is touched. */
int kws_frontend_linear_size(kws_frontend_handle h);
int kws_frontend_run_linear(kws_frontend_handle h, const float* pcm /*[B, n_max] device*/, const int32_t* n_samples /*[B] device or NULL*/,
                            int B, int n_max, float* spec /*[B, T_max, 201]*/, int32_t* frames_out /*[B]*/, float* energy_out /*[B]*/,
                            void* stream);
int kws_frontend_augment(kws_frontend_handle h, const float* spec, const int32_t* frames, const float* energy, int B, int T_max,
                         const float* noise_spec, const int32_t* noise_frames, const float* noise_energy, int K, int Tn_max,
                         const int32_t* src /*[R]*/, const int32_t* noise /*[R]*/, const int32_t* start /*[R]*/, const float* gain_db /*[R]*/,
                         int R, float* out /*[R, T_max, feature_size]*/, void* stream);

/* Device-side decode window of the streaming loop (detector.py:122,168-209; utils/queue.py): per stream a
 * bounded FIFO of up to `max_chunks` (1..64) softmax chunks (each <= max_frames frames; 2 * max_chunks *
 * round_up(max_frames, 16) bytes must fit 48 KiB, else KWS_ERR_UNSUPPORTED).  The frame ring behind kws_window_step is
 * allocated by its first call (a window that is only driven incrementally never holds one).  ctc_decode2's per-frame rule
 * (argmax over classes 1..C-2, strictly above `thres`) is a function of the frame alone, so the window stores each
 * frame's word rather than its softmax row; `thres` is therefore fixed per handle.  kws_window_step, per stream:
 *   clear_before[b] != 0 -> empty the window first (silence: detector.py:171-177);
 *   append softmax[b] (dropping the oldest chunk when full); ctc_decode2 over the concatenated window;
 *   hit[b] = label occurs in the decoded words (ctc_predict); on a hit the window is emptied and restart[b]=1
 *   (the caller passes it as the next kws_step reset_mask: detector.py:202-208). */
typedef struct kws_window* kws_window_handle;
int kws_window_create(int B, int max_chunks, int max_frames, int C, float thres, kws_window_handle* out);
int kws_window_destroy(kws_window_handle h);
int kws_window_step(kws_window_handle h, const float* softmax /*[B,T,C]*/, int T, const uint8_t* clear_before,
                    const char* label, int32_t* hit /*[B]*/, uint8_t* restart /*[B] or NULL*/, void* stream);

/* The same window step in incremental form: the window keeps a SUMMARY per queued chunk (first / last frame word and where the
 * label matcher ends up for each of its <= 16 entry states) instead of the chunk's frames, and evaluates the <= max_chunks
 * summaries, oldest first -- O(chunks) per step, not O(frames in the window).  Whether a chunk's first frame emits depends
 * on the chunk before it in the window, which is what an eviction changes: that one decision is taken at evaluation time, so
 * the result is exactly the re-scan's (property-tested against it, evictions / empty chunks / clears / triggers included:
 * tests/test_window_incremental.py, tests/test_gpu_window.py).  Same arguments and results as kws_window_step.  The summaries
 * are label-specific: the first call binds `label` to the window (uploads its matcher: synchronises once), later calls must
 * pass the same one (KWS_ERR_INVALID_ARGUMENT otherwise).  The incremental state is separate from kws_window_step's frame
 * ring: drive a window through ONE of the two entry points.  kws_stream_feed uses this form -- inside the last GRU layer's
 * launch where that kernel has the tail (fp32 / f16x3 / bf16 stacks at hidden = 128, chunks of <= 64 frames, windows of
 * <= 24 chunks) AND every workgroup takes one group of 16 streams (B <= 16 x the device's CUs: 4096 on 256 CUs); as a launch
 * of its own otherwise.  That launch stages 16 streams' frame words and rings in LDS: 16 * round_up(T, 16) + 256 +
 * 16 * (32 * max_chunks + 32) bytes must fit 160 KiB, else KWS_ERR_UNSUPPORTED (kws_window_create only sizes the re-scan). */
int kws_window_step_incremental(kws_window_handle h, const float* softmax /*[B,T,C]*/, int T, const uint8_t* clear_before,
                                const char* label, int32_t* hit /*[B]*/, uint8_t* restart /*[B] or NULL*/, void* stream);

/* The whole loop iteration of detector.py:158-209 for B streams as ONE call (device-side stream manager, native):
 *   data = ring_buffer.get()                      `pcm` [B,n]: float samples, or int16 PCM scaled by 2^-15 (:40-43,74-79)
 *   vad(data, vad_thres) false -> clean_state() + prob_queue.clear()                                   (:168-177)
 *   data = concatenate(res, data); res = data[-keep:]      carried samples, never materialised          (:179-183)
 *   softmax, state = sess.run(...)                 front-end + GRU stack on the carried state           (:190-196)
 *   prob_queue.add(softmax); ctc_decode2 over the window; ctc_predict(label)                            (:195-201)
 *   on a hit: window cleared, state reset requested for the next chunk                                  (:202-208)
 * i.e. kws_vad -> kws_frontend_run_carry -> kws_step -> kws_window_step_incremental with the mask logic fused into the first
 * kernel, the window step into the last, and no host work per stream: three launches per chunk (gate + front-end, two GRU
 * layers; two for the bf16 stack) when the window step rides in the last layer's launch (conditions above), one more
 * (window_inc_kernel) otherwise -- e.g. at B > 16 x CUs.  `label` is bound to `window` at kws_stream_create.  The handle
 * BORROWS the model, front-end and window handles (they should outlive it; a feed after one of them was destroyed fails with
 * KWS_ERR_INVALID_ARGUMENT) and the caller-owned device buffers `state` [L,B,H] (zero it to start) and `restart` [B] u8
 * (zero it).  It OWNS only the sample carry (2 x (fft_size - 1) floats per stream); one chunk's intermediates (mel, softmax,
 * masks) are carved out of a staging block of the MODEL handle that all its stream handles share, so M managers on one model
 * cost M x (state + carry + window summaries) -- about 4.8 KB per stream at the reference's shape -- not M x a chunk's
 * buffers.  An empty chunk (n == 0) is skipped as detector.py:164-166 does.  Fewer than
 * fft_size samples in total so far: the reference still runs its whole iteration on such a chunk, and so does this --
 * the VAD decision clears state and window, every sample is carried, the model runs over zero frames (state handed
 * back, or zeroed where the VAD said silence) and the empty softmax takes a slot of the window before the windowed
 * decode.  `label`: up to 15 digits '1'..'9' (the incremental window's matcher has 16 states). */
typedef struct kws_stream* kws_stream_handle;
int kws_stream_create(kws_handle model, kws_frontend_handle frontend, kws_window_handle window, int B, int max_chunk_samples,
                      float vad_thres, const char* label, float* state, uint8_t* restart, kws_stream_handle* out);
int kws_stream_destroy(kws_stream_handle h);
/* Forgets the carried samples (the model state, restart mask and window belong to the caller), and returns the handle to
 * lock-step mode (below).  Host-side only: no device work. */
int kws_stream_reset(kws_stream_handle h);
int kws_stream_feed(kws_stream_handle h, const void* pcm /*[B,n] device*/, int n, int pcm_int16, int32_t* hit /*[B] device*/,
                    void* stream);
/* Per-stream arrival (ragged chunks): the same iteration with stream b reading its own n_b = n_per_stream[b] samples, the
 * first n_b of row b of `pcm` [B, n_max] (samples at or past n_b are never read into a result; the padding may hold anything).
 * Each stream follows detector.py:158-209 on its own:
 *   n_b == 0                 the iteration is skipped for this stream only: no VAD, no reset, no window slot; its carry, GRU
 *                            state, window and restart[b] stay bitwise as they are; hit[b] = 0.  (A restart requested by an
 *                            earlier trigger waits for the stream's next non-empty chunk.)
 *   carry_b + n_b < fft_size VAD over the n_b samples, every sample carried, zero frames, an empty window slot (as above)
 *   otherwise                VAD, frames(carry_b + n_b) frames with this stream's reset mask, keep_b samples carried, one
 *                            window slot of those frames, decode, trigger.
 * The lengths stay on the device: no host read, no host wait (a caller may fill them on the device).  Values outside
 * [0, n_max] are CLAMPED to it; n_max itself must lie in [0, max_chunk_samples].  Needs the 400-point FFT front-end
 * (KWS_ERR_UNSUPPORTED otherwise).  A call with n_max == 0 skips every stream: it reads and writes nothing but `hit`, and
 * leaves the handle's mode (below) as it is.  Launches per call, whatever the lengths: the front-end with the per-stream gate, the GRU
 * layers with seq_len = each stream's frames (copy-through past them), and window_inc_kernel over each stream's own frames --
 * FOUR for the fp32 and f16x3 stacks, THREE for the bf16 stack (the window step cannot ride in the last GRU launch: those
 * instantiations take no lengths).  kws_last_launch reports the GRU launches.
 *
 * Mode switch.  A handle starts in LOCK-STEP mode: one carried length for all streams (kws_stream_feed as described above).
 * Its first kws_stream_feed_ragged or kws_stream_recycle moves it to PER-STREAM carry lengths (device array, no extra launch
 * in the feed); from then on kws_stream_feed(n) runs the ragged iteration with every n_b = n (the same results as lock-step
 * feeds would give).  kws_stream_reset returns it to lock-step mode with no carry.  Until a handle's first ragged feed or
 * recycle, kws_stream_feed runs exactly its lock-step code. */
int kws_stream_feed_ragged(kws_stream_handle h, const void* pcm /*[B,n_max] device*/, int n_max,
                           const int32_t* n_per_stream /*[B] device*/, int pcm_int16, int32_t* hit /*[B] device*/, void* stream);
/* Slot recycling: every stream b with slots[b] != 0 becomes what a freshly created manager's stream is -- carry length 0,
 * window emptied, state rows [l][b][:] zeroed, restart[b] = 0 -- for a new client taking over the slot.  The other streams stay
 * bitwise untouched.  One launch; switches the handle to per-stream carry lengths (above).  400-point FFT front-end only. */
int kws_stream_recycle(kws_stream_handle h, const uint8_t* slots /*[B] device, non-zero = recycle*/, void* stream);
/* The carried samples as they stand (detector.py:181-183's `res` of every stream), in either mode: stream b's
 * lengths[b] <= fft_size - 1 samples at samples[b * (fft_size - 1) ...]; the rest of each row is unspecified.  Copies only (no
 * kernel), ordered like a feed; changes nothing. */
int kws_stream_carry(kws_stream_handle h, float* samples /*[B, fft_size - 1] device*/, int32_t* lengths /*[B] device*/, void* stream);

/* A stream manager on a customised-keyword model (kws_create_heads): BOTH class heads decoded per chunk, the stack run once.
 * The reference README ("Customize keyword") keeps both dense layers on the frozen stack and says "do softmax and decode
 * respectively"; server_demo.py:122-129 ORs the two decisions.  Per chunk and stream, detector.py:158-209 applied per head:
 *   VAD      a silent chunk clears BOTH windows and resets the state (clear_before applies to both)
 *   stack    once; every layer writes its rows to a seam, as kws_step_heads plans it
 *   head k   its softmax rows go into window k, ctc_decode2 over the window at window k's threshold, hit_k = label_k occurs
 *   coupling fired = hit_1 | hit_2: BOTH windows are cleared and the restart is requested, whichever head fired
 *   output   hit[b] = hit_1 | hit_2 << 1 (0 nothing, 1 / 2 / 3 which head fired: non-zero is "detected")
 * A chunk that completes no frame puts an empty entry into both windows; a skipped stream of the ragged feed gets no slot in
 * either, hit 0, restart untouched.  Launches per chunk: front-end + L layers + 1 -- heads_window_kernel behind the stack does both
 * projections, both softmaxes, both windows and the coupling (kws_last_launch names it in the top layer's slot, and with profiling
 * on it is timed there); lock-step and ragged feeds alike.  It stages a 32-frame block of logits (32 KiB), both heads' frame words
 * (2 * 16 * round_up(T, 16) bytes), two label tables and the two windows' rings (16 * (32 * max_chunks + 32) bytes each) in LDS:
 * more than 160 KiB is refused with KWS_ERR_UNSUPPORTED and the byte counts.
 *   kws_stream_create_heads   as kws_stream_create, with `window1` (C = num_classes, label1) and `window2` (C = num_classes2,
 *                             label2): each window is bound to its own label.  Refuses (KWS_ERR_INVALID_ARGUMENT) a model without
 *                             a second head, a window whose C or B does not fit its head, windows that hold fewer frames per
 *                             chunk than max_chunk_samples gives, bad labels, and everything kws_stream_create refuses.  The
 *                             handle is a stream handle: kws_stream_feed / _feed_ragged / _recycle (empties both windows of a
 *                             recycled stream; two launches) / _carry / _reset / _destroy take it.  A feed stages nothing beyond
 *                             what kws_reserve sizes for a heads step, and never allocates.  kws_stream_create on the same model
 *                             handle stays what it is -- head 1 through the fused tail -- and both kinds of handle may coexist.
 *   kws_step_heads_window     the same iteration from mel on: kws_step_heads' stack on `mel` [B,T,n_mel] (T >= 0) with `reset_mask`,
 *                             then the one launch on the two windows (`clear_before` [B] or NULL).  softmax1 [B,T,num_classes] /
 *                             softmax2 [B,T,num_classes2], each or NULL: bitwise the rows kws_step_heads writes for the same mel
 *                             and state.  restart [B] or NULL.  The labels are bound to the windows as kws_window_step_incremental
 *                             binds them; mel-fed and PCM-fed chunks may alternate on the same windows.
 * Out of scope: f16x3 / bf16 / int8 heads and the cell wrappers (kws_create_heads refuses them), more than two heads, the MFCC and
 * dataset front-ends. */
int kws_stream_create_heads(kws_handle model, kws_frontend_handle frontend, kws_window_handle window1, kws_window_handle window2, int B,
                            int max_chunk_samples, float vad_thres, const char* label1, const char* label2, float* state, uint8_t* restart,
                            kws_stream_handle* out);
int kws_step_heads_window(kws_handle model, const float* mel, const float* state_in, float* state_out, const uint8_t* reset_mask, int B, int T,
                          kws_window_handle window1, kws_window_handle window2, const char* label1, const char* label2,
                          const uint8_t* clear_before, float* softmax1, float* softmax2, int32_t* hit /*[B]*/, uint8_t* restart, void* stream);

/* Customised-keyword enrolment (README "Customize keyword"; models/rnn_ctc.py:59-101): the GRU stack and every column of the trained
 * [H, C] projection stay frozen, n_new columns [H, n_new] and their bias are trained on a few utterances with tf.nn.ctc_loss and
 * tf.train.AdamOptimizer, and stand in front of the blank column of the second head (kws_create_heads).  The stack runs ONCE
 * (kws_step_heads: nn_outputs and head 1's logits, which are the second head's frozen logits); every optimiser step after that is
 * the fit below.
 *
 * The CTC loss (both entry points): the blank is the LAST class; labels index classes 0..classes-2; extended label sequence blank,
 * l_1, blank, ..., l_S, blank with S <= 31.  Frames t >= seq_len[b] contribute nothing.  seq_len[b] == 0 is an empty slot: loss 0,
 * gradient 0, its label ignored.  An utterance without a valid path (seq_len < S + repeats) has loss +inf and gradient exactly 0.
 * seq_len [B], labels [B,S_max] and label_len [B] are HOST memory: they are range-checked before anything is launched
 * (KWS_ERR_INVALID_ARGUMENT) and reach the device as one stream-ordered copy.  LDS: 4 T (8 + 2 S_max + 1) bytes per utterance; more
 * than 160 KiB per workgroup is KWS_ERR_UNSUPPORTED with the byte counts.
 *
 *   kws_ctc_loss   logits [B,T,C] f32 device, C in 3..8 -> loss [B] (-log P) and, unless NULL, grad_logits [B,T,C] = softmax -
 *                  occupancy / P, zero at t >= seq_len[b].  One wave per utterance. */
int kws_ctc_loss(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C, int S_max,
                 float* loss, float* grad_logits_or_null, void* stream);
/* CTC forced alignment: given the transcript, where in the utterance each label lies and how sure the model is of it.  kws_ctc_loss's
 * conventions: logits [B,T,C] f32 device, C in 3..8, the blank is the LAST class, extended label blank, l_1, blank, ..., l_S, blank with
 * S <= 31 and L = 2S + 1 states; seq_len [B], labels [B,S_max], label_len [B] are HOST memory, range-checked before anything is launched
 * and shipped as one stream-ordered block; frames t >= seq_len[b] are never read.  One wave per utterance; stateless, stream-ordered,
 * allocates only that block, never synchronises.
 *   score  [B] f32 out (required): the log-probability of the best single path through the extended label -- the loss's recursion over the
 *          log-softmax rows with max in place of log-add-exp (Viterbi).
 *   states [B,T] i32 out or NULL: that path's state at every frame, 0..2S (even: a blank, 2k+1: label k); -1 at t >= seq_len[b].
 *   spans  [B,S_max,2] i32 out or NULL: first and last frame (inclusive) the path spends in label k (state 2k+1); -1 at k >= label_len[b].
 *          On a valid path every label has a span, and the spans are disjoint and increasing.
 *   loss   [B] f32 out or NULL: -log P(label), bit-identical to kws_ctc_loss's value on the same arguments.
 *   post   [B,T,S_max] f32 out or NULL: the posterior occupancy of label state 2k+1 at frame t given the label, exp(alpha + beta - lp +
 *          loss) clamped to 1 -- the quantity kws_ctc_loss's gradient sums per class --, in [0,1]; 0 at t >= seq_len[b] and at
 *          k >= label_len[b].  The blank states are not written: their total at a frame is 1 - sum_k post[b,t,k].
 * Ties, so that one input always gives the same bits: at every (frame, state) a predecessor replaces the current choice only when it is
 * strictly greater, tried in the order stay, s-1, s-2 (s-2 only between different labels); the path ends in state L-1 unless L-2 is
 * strictly greater.
 *   seq_len[b] == 0 (an empty slot, its label ignored):  score 0, loss 0, states -1, spans -1, post 0.
 *   no valid path (seq_len < S + repeats):                score -inf, loss +inf, states -1, spans -1, post 0.
 * LDS per utterance: 4 T (13 + A) bytes -- 8 log-probabilities, 4 words of back-pointers and 1 state per frame, and A = 2 S_max + 1
 * states of alpha when loss or post is asked for, A = 0 otherwise.  Every refusal is decided before the device is probed: a NULL among
 * the required pointers, the ranges above, a pointer that is not 4-byte aligned, a length or label out of range
 * (KWS_ERR_INVALID_ARGUMENT); more than 160 KiB of LDS (KWS_ERR_UNSUPPORTED with the byte counts). */
int kws_ctc_align(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C, int S_max,
                  int32_t* states_or_null, int32_t* spans_or_null, float* score, float* loss_or_null, float* post_or_null, void* stream);
/* An enrolment handle: E independent enrolments of K utterance slots each (K in 1..4, B = E*K utterances, enrolment e owns
 * utterances e*K .. e*K+K-1), for a model of hidden size H (64, 128, 256) whose trained head has C classes (3..7) and n_new new
 * ones (C + n_new <= 8).  It owns the new columns Wn [E,H,n_new], their bias bn [E,n_new], Adam's two moments and the step count.
 *   kws_enroll_set    Wn, bn (device) -> the handle; zeroes the moments and the step count
 *   kws_enroll_fit    `iterations` optimiser steps in ONE launch, one workgroup per enrolment.  nn_outputs [B,T,H] and logits1 [B,T,C]
 *                     (device): what kws_step_heads returns for the utterances, of a model without use_relu / value_clip.  Per step:
 *                     logits2 = (logits1[.., 0..C-2] | nn_outputs . Wn + bn | logits1[.., C-1]), the CTC loss of every slot on
 *                     `labels` (which index the C + n_new classes of that head), its gradient with respect to Wn and bn summed over
 *                     the K slots in slot order and divided by K (config.batch_size; empty slots add 0), then TensorFlow's Adam:
 *                     lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t), theta -= lr_t m / (sqrt(v) + 1e-8); no gradient clipping.
 *                     loss_trace [iterations, B] (device) or NULL: every slot's loss at every step, before that step's update.
 *                     N calls of one iteration give the bits of one call of N.
 *   kws_enroll_fit_frames  the same fit on frame-wise targets, alone or mixed with the CTC loss ("Frame-wise targets" below)
 *   kws_enroll_get    the handle's Wn, bn -> device buffers
 *   kws_enroll_moments  Adam's m and v, each [E,H,n_new] followed by [E,n_new], -> device buffers (inspection / tests)
 *   kws_enroll_stats  device bytes the handle holds, device (re)allocations since create (one at the first fit of a shape; each
 *                     waited for the device) and optimiser steps since kws_enroll_set; any pointer may be NULL
 * One host thread at a time per handle (KWS_ERR_BUSY); a call on another stream than the previous one is ordered behind it by the
 * handle's event.  No call synchronises except create, destroy and the first fit at a larger B * (2 + S_max). */
typedef struct kws_enroll* kws_enroll_handle;
int kws_enroll_create(int H, int C, int n_new, int E, int K, kws_enroll_handle* out);
int kws_enroll_destroy(kws_enroll_handle h);   /* always KWS_OK */
int kws_enroll_set(kws_enroll_handle h, const float* Wn, const float* bn, void* stream);
int kws_enroll_fit(kws_enroll_handle h, const float* nn_outputs, const float* logits1, const int32_t* seq_len, const int32_t* labels,
                   const int32_t* label_len, int T, int S_max, float lr, int iterations, float* loss_trace_or_null, void* stream);
int kws_enroll_get(kws_enroll_handle h, float* Wn, float* bn, void* stream);
int kws_enroll_moments(kws_enroll_handle h, float* m, float* v, void* stream);
int kws_enroll_stats(kws_enroll_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps);

/* CTC prefix beam search: the top_paths best labellings of every utterance and their log-probabilities (the decoder both graphs of
 * models/rnn_ctc.py leave commented out: tf.nn.ctc_beam_search_decoder(log(softmax), seqLengths, beam_width=config.beam_size,
 * top_paths=1)).  One wave per utterance; stateless, stream-ordered, allocates nothing, never synchronises.
 *   logits   [B,T,C] f32 device, 16-byte aligned, C in 3..8.  The kernel takes the log-softmax of each row itself, so raw logits and
 *            log(softmax) give the same result.  The blank is the LAST class; labels are 0..C-2.
 *   seq_len  [B] i32 DEVICE memory, or NULL for T; values are clamped to 0..T, frames t >= seq_len[b] are never read.
 *   The beam is a set of at most beam_width (1..32) label prefixes, each with (lp_b, lp_nb): the log-probability of the paths that
 *   collapse to it and end in the blank / in a label; it starts as the empty prefix at (0, -inf).  Per frame every prefix p stays
 *   (lp_b' += (lp_b + lp_nb) lp[blank]; lp_nb' += lp_nb lp[last(p)]) and is extended by every label c unless len(p) == L_max
 *   (p+c: lp_nb' += lp[c] (lp_b if c == last(p), else lp_b + lp_nb); sums and products of probabilities, computed in the log domain).
 *   Candidates with the same prefix merge, however they arose -- identity is the prefix's content -- and the beam_width candidates with
 *   the largest lp_b' + lp_nb' survive; ties go to the smaller candidate index (8 x beam slot + label, the stay last), so one input
 *   always gives the same bits.  This is the exact-candidate form: TensorFlow's decoder prunes further once its beam is full; with
 *   beam_width >= the number of labellings the two coincide.
 *   paths    [B,top_paths,L_max] i32 out: rank k's labels, -1 past the end; L_max in 1..64, top_paths in 1..beam_width
 *   lengths  [B,top_paths] i32 out
 *   log_prob [B,top_paths] f32 out, descending: log(P_b + P_nb) of the prefix.  Ranks past the prefixes that exist: length 0, all -1,
 *            -inf.  seq_len[b] == 0: the empty prefix with log_prob 0 at rank 0.
 *   merge_repeated != 0 drops a label equal to its predecessor as the path is written (tf.nn.ctc_beam_search_decoder's output option,
 *            on by default there); the scores are untouched.
 * Every refusal (null pointers, the ranges above, B or T < 1, alignment: KWS_ERR_INVALID_ARGUMENT; 32 T + 7552 bytes of LDS above
 * 160 KiB: KWS_ERR_UNSUPPORTED with the byte counts) is decided before the device is probed. */
int kws_ctc_beam_search(const float* logits, const int32_t* seq_len_or_null, int B, int T, int C, int beam_width, int top_paths, int L_max,
                        int merge_repeated, int32_t* paths, int32_t* lengths, float* log_prob, void* stream);

/* Per-user customised keywords: ONE bank of enrolled heads behind one frozen model.  kws_enroll_fit produces one set of columns per
 * user; a heads handle bakes one second head into the model.  A bank keeps `capacity` slots of n_new columns Wn[u] [H, n_new] and their
 * bias bn[u] [n_new] on the device (all zero at creation) for a model of hidden size H (64 / 128 / 256) whose trained head has C classes
 * (3..7, C + n_new <= 8), and a step takes user [B] int32 (device): the slot of each stream.
 *   stream b, u = user[b] in [0, capacity):  head 1 is exactly head 1 of kws_step_heads.  Head 2 has C2 = C + n_new classes: head 1's
 *       logits for classes 0..C-2, then nn_outputs[b,t,:] . Wn[u] + bn[u], then head 1's blank logit (kws_enroll_fit's splice); on that
 *       row relu / clip, softmax and the ctc_decode2 frame rule at head 2's own threshold.
 *   user[b] outside [0, capacity) (-1 by convention; any other out-of-range value reads as -1, nothing is read out of bounds):  the
 *       stream has no second head -- its logits2 / softmax2 rows are zeros, its head-2 tokens are 0, its head-2 prev_word becomes -1;
 *       in a stream manager window 2 takes its chunk entries like any other, all of them wordless, so hit_2 is never set: the stream
 *       behaves exactly as a stream of a plain one-head manager.
 *   rows past seq_len[b]:  as kws_step_heads -- nn_outputs 0, head 1 = bfc, head 2's new classes = bn[u], no word.
 *   kws_bank_create   range refusals (KWS_ERR_UNSUPPORTED for H, KWS_ERR_INVALID_ARGUMENT for C / n_new / capacity < 1) are decided
 *                     before the device is probed.
 *   kws_bank_set      slots [first, first + count) <- Wn [count,H,n_new], bn [count,n_new] (device): the layout kws_enroll_get writes,
 *                     so enrol -> serve is two calls and no host copy.  Stream-ordered; the caller orders it against the feeds that
 *                     read those slots.  first + count > capacity is refused.
 *   kws_bank_get      the same slots -> device buffers (tests).
 *   kws_step_bank     kws_step_heads with head 2 from the bank.  `model` is a kws_create_heads handle (its plan, seams and side buffers
 *                     serve the step, so kws_reserve covers it unchanged; its OWN second head is not read); the bank's H and C are the
 *                     model's.  head2 rows have C + n_new classes.  Everything else as kws_step_heads.  kws_last_launch names
 *                     bank_heads_kernel<H/16> in the top layer's slot, and profiling times it there.
 *   kws_stream_create_bank   kws_stream_create_heads with head 2 from the bank: window2 has C + n_new classes; `user` [B] (device) is
 *                     borrowed like state / restart -- the caller rewrites user[b] on the device when a slot is recycled for a new
 *                     client.  The policy is kws_stream_create_heads' unchanged (silence clears both windows and resets the state;
 *                     fired = hit_1 | hit_2 clears both and requests the restart; hit[b] = hit_1 | hit_2 << 1; a zero-frame chunk puts
 *                     an empty entry into both windows; a skipped stream of the ragged feed gets no slot in either).  label2 is
 *                     bound to window 2 and is the pattern of every slot WITHOUT a keyword of its own: with a fixed n_new the new words
 *                     are classes C-1 .. C+n_new-2 for every user, so "56" is everybody's keyword pattern over their own columns;
 *                     users whose keyword has another word pattern or fewer new words set it on their slot (kws_bank_set_keyword) and
 *                     share the manager.  The handle is a stream handle (kws_stream_feed / _feed_ragged / _recycle /
 *                     _carry / _reset / _destroy); recycling does what it does on a heads manager.  The launch stages the group's
 *                     columns (16 H n_new floats + 512 bytes) next to what heads_window_kernel stages: more than 160 KiB of LDS is
 *                     KWS_ERR_UNSUPPORTED with the byte counts.
 *   kws_step_bank_window     kws_step_heads_window with `bank, user` added (mel-fed); softmax2 rows are bitwise kws_step_bank's.
 *   kws_bank_set_keyword     slot `slot` gets a keyword of its own: its head 2 has C + n_used classes (1 <= n_used <= n_new: trained classes
 *                     0..C-2, the slot's first n_used columns, the blank), and window 2 of every stream on that slot matches `label`
 *                     instead of the manager's label2.  logits2 / softmax2 rows keep C + n_new entries, those past C + n_used - 1 are 0;
 *                     the word and the tokens come from the C + n_used row.  label == NULL: back to "no keyword of its own" (n_used must
 *                     then be n_new).  Refused before the device is touched (KWS_ERR_INVALID_ARGUMENT): slot outside [0, capacity),
 *                     n_used outside [1, n_new], a label of more than 15 digits (the matcher has 16 states), a digit outside '1'..'9',
 *                     a digit d > C + n_used - 2 (a word class the slot's head does not have: it could never fire).  Stream-ordered
 *                     like kws_bank_set.  From the first keyword on, every launch on the bank takes the keyword form of its kernel --
 *                     kws_last_launch names bank_keyword_heads_kernel<H/16> / bank_keyword_window_kernel<H/16> -- which stages the group's
 *                     sixteen matchers (4 KiB + 128 bytes of LDS more; counted in the 160 KiB refusal); a bank on which no keyword
 *                     was ever set launches the kernels it always did.
 *   kws_bank_get_keyword     what the slot was last given: *n_used, label[16] ("" and *own = 0 when it has none).  Host state, no device
 *                     access.
 * Window 2's chunk summaries are built with the matcher of the moment, which the library cannot check: after rewriting user[b] to a slot
 * with another keyword, or after kws_bank_set_keyword on a slot that live streams use, the caller recycles those streams
 * (kws_stream_recycle) before their next feed.
 * One host thread at a time per bank (KWS_ERR_BUSY) in kws_bank_set / _get / _set_keyword / _get_keyword, kws_step_bank and kws_step_bank_window.  The feeds of a bank
 * manager (kws_stream_feed / _feed_ragged) do NOT take the bank's guard: they only queue launches that read the bank's fixed device
 * block, so a kws_bank_set from another thread is ordered against them by the caller, on the stream, like any other writer of memory
 * a feed reads.  Out of scope: more than two heads, per-user decode thresholds, labels for head 1, and
 * whatever kws_create_heads refuses (f16x3 / bf16 / int8 stacks, the cell wrappers). */
typedef struct kws_bank* kws_bank_handle;
int kws_bank_create(int H, int C, int n_new, int capacity, kws_bank_handle* out);
int kws_bank_destroy(kws_bank_handle bank);   /* always KWS_OK */
int kws_bank_set(kws_bank_handle bank, int first, int count, const float* Wn /*[count,H,n_new] device*/, const float* bn /*[count,n_new] device*/,
                 void* stream);
int kws_bank_get(kws_bank_handle bank, int first, int count, float* Wn, float* bn, void* stream);
int kws_bank_set_keyword(kws_bank_handle bank, int slot, int n_used, const char* label, void* stream);
int kws_bank_get_keyword(kws_bank_handle bank, int slot, int* n_used, char* label /*[16]; "" + *own = 0 when none*/, int* own);
int kws_step_bank(kws_handle model, kws_bank_handle bank, const int32_t* user /*[B] device*/, const float* mel, const float* state_in,
                  float* state_out, const int32_t* seq_len, const uint8_t* reset_mask, float* nn_outputs, const kws_head_io* head1,
                  const kws_head_io* head2, int B, int T, void* stream);
int kws_stream_create_bank(kws_handle model, kws_frontend_handle frontend, kws_window_handle window1, kws_window_handle window2,
                           kws_bank_handle bank, const int32_t* user /*[B] device*/, int B, int max_chunk_samples, float vad_thres,
                           const char* label1, const char* label2, float* state, uint8_t* restart, kws_stream_handle* out);
int kws_step_bank_window(kws_handle model, kws_bank_handle bank, const int32_t* user /*[B] device*/, const float* mel, const float* state_in,
                         float* state_out, const uint8_t* reset_mask, int B, int T, kws_window_handle window1, kws_window_handle window2,
                         const char* label1, const char* label2, const uint8_t* clear_before, float* softmax1, float* softmax2,
                         int32_t* hit /*[B]*/, uint8_t* restart, void* stream);

/* Training of the stack itself (main.py's training loop on models/rnn_ctc.py:34-101,179-284): the L-layer GRU and the class projection
 * under tf.nn.ctc_loss, with tf.clip_by_global_norm and tf.train.AdamOptimizer or MomentumOptimizer(0.9, use_nesterov=True).  A train
 * handle owns the parameters (the canonical blob of kws_weights_nbytes, on the device), the optimiser's moments and the step count.
 *
 * The graph of one step, from the zero state (initial_state=None; from a carried state: kws_train_grad_state, below):
 *   layer l     TF 1.x GRUCell as kws_step computes it: [r,u] = sigma([x,h].Wg + bg), c = tanh([x, r o h].Wc + bc), h' = u o h + (1-u) o c;
 *               dynamic_rnn(sequence_length): at t >= seq_len[b] the state is copied and the output is 0
 *   dropout     DropoutWrapper(output_keep_prob): the layer's output is y = h' o mask / keep_prob, the carried state the undropped h'.
 *               drop: uint8 [L,B,T,H] on the device (0 = dropped), 4-byte aligned (the kernels read four units' masks at a time), or NULL for none.  Input dropout is the caller's (on x, no gradient).
 *               On a kws_train_create_wrapped handle with variational_recurrent = 1, drop is uint8 [L,B,H]: one mask per stream and layer,
 *               held for all frames (DropoutWrapper(variational_recurrent=True), models/rnn_ctc.py:191-195) -- the same arithmetic.
 *   loss        logits = y_top . Wfc + bfc; loss = sum_b ctc_b / B with kws_ctc_loss's conventions (above): the blank is the last class,
 *               S_max <= 31, seq_len / labels / label_len are HOST arrays range-checked before any launch, seq_len[b] == 0 is an empty slot
 *               that adds 0 and still counts in B.  An utterance without a valid path has loss +inf and contributes a gradient of exactly 0;
 *               its loss[b] is +inf, so the step loss sum(loss) / B a caller forms is +inf as well.
 *   clipping    only when max_grad_norm > 0: g *= max_grad_norm / max(||g||_2, max_grad_norm) over all tensors
 *   Adam        beta 0.9 / 0.999, eps 1e-8 outside the root, lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t) (as kws_enroll_fit)
 *   Nesterov    a <- 0.9 a + g; theta <- theta - lr g - lr 0.9 a
 * The learning rate is an argument of every step (the exponential-decay schedule is host arithmetic).
 *
 * Backward, frames in reverse, dh' = dy o mask / keep_prob + the carried dh:
 *   du = dh' o (h - c), dc = dh' o (1 - u), dh = dh' o u;  dc^ = dc o (1 - c^2);  [dx_c | d(rh)] = dc^ . Wc^T;  dh += d(rh) o r;
 *   dr^ = d(rh) o h o r (1 - r);  du^ = du o u (1 - u);  [dx_g | dh_g] = [dr^ | du^] . Wg^T;  dh += dh_g;  dx = dx_c + dx_g;
 *   dWc += [x, r o h]^T dc^;  dWg += [x, h]^T [dr^ | du^];  the biases are the column sums.  Frames t >= seq_len[b] pass dh through.
 * Nothing is summed with float atomics: the same call twice gives the same bits.
 *
 * The cell wrappers (kws_train_create_wrapped; kws_cell_wrappers above): the graph of a layer is Residual(Dropout(LayerNormalizer(GRUCell))),
 * the residual on layers >= 1 only.  M = B T rows, in_l the input of layer l (x, or out_{l-1}) of width I_l, k = 0.7071067811865475;
 * rows t >= seq_len[b] are written as zeros and never read (the padding of x may be NaN), and add exactly 0 to every sum.
 *   layer norm  m = mean(in_l), v = mean((in_l - m)^2), rstd = 1 / sqrt(v + 1e-5), xn = (in_l - m) rstd, x^ = xn ibeta_l + igamma_l: the
 *               cell's x-part reads x^ (ibeta the scalar scale, igamma the per-feature shift, as in kws_create_wrapped)
 *   residual    out_l = k (y_l + in_l) for l >= 1, y_l the layer's output after dropout; the state stays the cell's; the dense layer reads
 *               out_{L-1}
 *   backward    given dout_l: with the residual dy_l = k dout_l enters the frame loop.  g = [dr^ | du^ | dc^] . (Wg_x | Wc_x)^T is dx^_l
 *               (with the layer norm on layer 0 too); dn = g ibeta, a = mean(dn), c = mean(dn o xn):
 *               d in_l = rstd (dn - a - xn c), d ibeta_l = sum over rows and features of g o xn, d igamma_l = sum over rows of g; without
 *               the layer norm d in_l = g.  With the residual k dout_l is added to d in_l; the sum is dout_{l-1}.  The x rows of dWg and
 *               dWc are taken with x^ in the place of in_l.
 *   parameters  ibeta and igamma are trained like every other tensor: they lie behind the canonical blob as in kws_weights_nbytes_wrapped
 *               (weights, gradient and both moments), enter the global norm and the clip, and take the same update.
 *
 * kws_train_create   refuses, before the device is probed, with KWS_ERR_UNSUPPORTED and a message that names the field: model.use_relu /
 *                    model.value_clip (the gradient of TensorFlow's relu and clip at their ties is not pinned), wrappers.use_layer_norm /
 *                    wrappers.use_residual, variational_recurrent (all three: kws_train_create_wrapped takes them, and the message says
 *                    so), any model.precision but KWS_FP32, keep_prob outside (0, 1]; with
 *                    KWS_ERR_INVALID_ARGUMENT an unknown optimizer and the ranges of kws_config (hidden 64 / 128 / 256, 1..8 layers,
 *                    n_mel 1..1024, 3..8 classes).  The parameters start as zeros: kws_train_set_weights comes first.
 * kws_train_create_wrapped   the same struct with wrappers.use_layer_norm, wrappers.use_residual and variational_recurrent each 0 or 1, in any
 *                    combination (another value: KWS_ERR_INVALID_ARGUMENT, naming the field); every other refusal of kws_train_create holds.
 *                    With all three 0 it is kws_train_create: the same launches, the same bits.  Every kws_train_* call below takes either
 *                    kind of handle; the blobs of a wrapped handle have kws_weights_nbytes_wrapped(&cfg.model, &cfg.wrappers) bytes.
 *                    kws_train_check_wrapped is kws_train_check for such a handle.
 * kws_train_check    the refusals of kws_train_create and of a kws_train_grad / _step call on a handle of this config, decided from
 *                    host memory alone: KWS_OK where the call would go on to the device.  x and loss are only compared with NULL and
 *                    checked for alignment.
 * kws_train_set_weights / _get_weights   the canonical blob in HOST memory (nbytes = kws_weights_nbytes(&cfg.model)); set zeroes the
 *                    moments and the step count.  Both wait for `stream`.
 * kws_train_reserve  sizes the handle's tape for calls up to this B, T, S_max (else the first call of a larger shape does: either waits
 *                    for the device once and counts in kws_train_stats' allocs).  A tape the device cannot hold is KWS_ERR_OUT_OF_MEMORY
 *                    with the byte counts, before anything is freed or allocated.
 * kws_train_grad     x [B,T,n_mel] f32 device; loss [B] f32 device out: every utterance's -log P; grad_blob (device, the blob's layout and
 *                    size) out: the gradient of sum(loss) / B BEFORE clipping; logits [B,T,C] device out or NULL (rows t >= seq_len[b] are
 *                    bfc).  Changes neither the parameters nor the moments.
 * kws_train_step     the same forward and backward, then clip and update with learning rate lr; grad_norm (device, one float) or NULL:
 *                    the global norm before clipping.  One call is one optimiser step.
 * kws_train_moments  the optimiser's slots -> HOST memory, blob layout each: Adam's m and v; Nesterov's accumulator in m, v zeros
 * kws_train_stats    device bytes the handle holds; device (re)allocations since create; optimiser steps since set_weights; kernel
 *                    launches of the last grad / step call; rows per chunk of the weight-gradient reduction for the last shape (the B*T
 *                    rows are summed in chunks of this many, the chunks in order).  Any pointer may be NULL.
 * Refused before the device is touched (KWS_ERR_INVALID_ARGUMENT): null pointers, B or T < 1, S_max outside [0, 31], labels / lengths out
 * of range, lr not positive and finite, pointers (drop included) not 4-byte aligned; KWS_ERR_UNSUPPORTED: 4 T (8 + 2 S_max + 1) bytes of LDS above 160 KiB,
 * as kws_ctc_loss.  One host thread at a time per handle (KWS_ERR_BUSY); a call on another stream than the previous one is ordered behind
 * it by the handle's event; no call synchronises the device in the steady state.
 *
 * Carried states (kws_train_grad_state / kws_train_step_state; kws_train_state_io below).  The graph above starts every layer from
 * state_in[l] in the place of zeros (initial_state of models/rnn_ctc.py:202-244) and hands out state_out[l], the state of layer l after
 * frame seq_len[b] - 1: [L,B,H] fp32 on the device as kws_step's, the carried state the undropped h' (dropout, above).  The objective is
 *   J = sum_b ctc_b / B + <dstate_out, state_out>
 * with dstate_out [L,B,H] the gradient of whatever the caller computes from state_out (NULL: zeros).  grad_blob is dJ / d parameters and
 * dstate_in [L,B,H] is dJ / d state_in: the backward loop's dh starts from dstate_out[l] and what is left of it in front of frame 0 is
 * dstate_in[l].  The formulas do not change; the h of frame 0 is state_in.
 *   chains      a recording cut into segments: run segment A, run B from A's state_out, run A again with dstate_out = B's dstate_in; the sum
 *               of the two grad_blobs is the gradient of the whole recording's loss, A's dstate_in that of A's state_in (A's forward runs
 *               twice: 1.5 x the cost of one pass).  Forward alone, A then B gives the logits and the final state of one call bit for bit:
 *               no frame's arithmetic depends on T.
 *   seq_len     a stream with seq_len[b] == 0, and every stream of a workgroup that runs no frame, copies state_in[b] to state_out[b] and
 *               dstate_out[b] to dstate_in[b] bit for bit.  Rows b >= B do not exist: nothing is written behind [L,B,H].
 *   no path     an utterance without a CTC path still adds exactly 0 from its loss; its state_out is computed and dstate_out still flows
 *               back through its frames into grad_blob and dstate_in.
 *   wrappers    both kinds of handle take the calls; layer norm, residual and dropout never touch the state.
 *   pointers    each of the four may be NULL; state_out may be state_in and dstate_in may be dstate_out (a lane reads its 16 bytes before
 *               the frame loop and writes the same 16 bytes behind it); no other overlap.  Each must be 16-byte aligned
 *               (KWS_ERR_INVALID_ARGUMENT naming the field, before the device is touched).
 * io == NULL, or all four fields NULL, is kws_train_grad / kws_train_step: the same launches, the same bits.  Otherwise the two frame loops of
 * every layer run in their state form: as many launches as the plain call (kws_train_stats), the loads and stores outside the frame
 * loops.  kws_train_step_state applies the gradient of J, dstate_out included.  Every refusal, KWS_ERR_BUSY, the ordering across streams
 * and "nothing synchronises in the steady state" are the plain calls'.
 * kws_train_check_state   the refusals of kws_train_create (wrapped != 0: of kws_train_create_wrapped) and of a _state call with this io,
 *                    from host memory alone.
 * kws_train_apply    one optimiser step from a gradient the caller supplies (device, the blob's layout and size; the sum of a chain's
 *                    gradients, of accumulated batches or of several devices): tf.clip_by_global_norm over it, then Adam or Nesterov with
 *                    the handle's moments and step count, then the packed weights -- what kws_train_step does behind its own gradient, bit
 *                    for bit when fed kws_train_grad's.  grad_norm as kws_train_step's.  Refused: NULL grad_blob, lr not positive and
 *                    finite, pointers not 4-byte aligned.  Three launches.
 * Out of scope: a learned initial state owned by the handle (the stream managers reset to zeros on the device: serving one would touch
 * every serving kernel family), the attention trainer, anything but fp32. */
enum { KWS_OPT_ADAM = 0, KWS_OPT_NESTEROV = 1 };
typedef struct kws_train_config {
    kws_config model;
    kws_cell_wrappers wrappers;       /* kws_train_create: both must be 0; kws_train_create_wrapped: each 0 or 1 */
    int32_t variational_recurrent;    /* kws_train_create: must be 0; kws_train_create_wrapped: 1 = one mask per stream, drop [L,B,H] */
    int32_t optimizer;                /* KWS_OPT_ADAM / KWS_OPT_NESTEROV */
    float max_grad_norm;              /* <= 0: no clipping (config/rnn_config.py:55: -1) */
    float keep_prob;                  /* output keep probability the masks were drawn with, (0, 1] */
} kws_train_config;
typedef struct kws_train* kws_train_handle;
size_t kws_sizeof_train_config(void);
int kws_train_create(const kws_train_config* cfg, kws_train_handle* out);
int kws_train_check(const kws_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                    int T, int S_max, const float* loss);
int kws_train_create_wrapped(const kws_train_config* cfg, kws_train_handle* out);
int kws_train_check_wrapped(const kws_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                            int B, int T, int S_max, const float* loss);
int kws_train_destroy(kws_train_handle h);   /* always KWS_OK */
int kws_train_set_weights(kws_train_handle h, const void* blob /*host*/, size_t nbytes, void* stream);
int kws_train_get_weights(kws_train_handle h, void* blob /*host*/, size_t nbytes, void* stream);
int kws_train_reserve(kws_train_handle h, int B, int T, int S_max);
int kws_train_grad(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null, void* stream);
int kws_train_step(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null, void* stream);
int kws_train_moments(kws_train_handle h, float* m /*host*/, float* v /*host*/, void* stream);
int kws_train_stats(kws_train_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches, int32_t* chunk_rows);
typedef struct kws_train_state_io {
    const float* state_in;    /* [L,B,H] f32 device, or NULL = the zero state */
    float*       state_out;   /* [L,B,H] out, or NULL; may alias state_in */
    const float* dstate_out;  /* [L,B,H] device, or NULL = zeros: gradient of the caller's objective w.r.t. state_out */
    float*       dstate_in;   /* [L,B,H] out, or NULL; may alias dstate_out */
} kws_train_state_io;
size_t kws_sizeof_train_state_io(void);
int kws_train_grad_state(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                         int T, int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null,
                         const kws_train_state_io* io_or_null, void* stream);
int kws_train_step_state(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                         int T, int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null,
                         const kws_train_state_io* io_or_null, void* stream);
int kws_train_check_state(const kws_train_config* cfg, int wrapped, const float* x, const int32_t* seq_len, const int32_t* labels,
                          const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_train_state_io* io);
int kws_train_apply(kws_train_handle h, const float* grad_blob /*device, blob layout*/, float lr, float* grad_norm_or_null, void* stream);

/* OctbitMatMul: out[A,N] = (sum_k u8(x)[a,k] * Wq[n,k] - signed*bias[n]) * scale_w * s_x.
 *   x [A,K] f32, Wq [N,K] s8 (pre-transposed), bias [N] f32, out [A,N] f32.  K % 64 == 0, scale_w > 0.
 *   per_row_scale = 0: one dynamic activation range over the whole x (the reference op, whose A is
 *   1 in streaming);  1: one range per row a (what a batch of independent streams needs to
 *   reproduce the batch-1 result).  The u8*s8 pair sums saturate to int16 as _mm_maddubs_epi16 does. */
int kws_octbit_matmul(const float* x, const int8_t* Wq, float scale_w, const float* bias, float* out,
                      int A, int K, int N, int per_row_scale, void* stream);

/* Host-side quantiser: W [K,N] f32 (host) -> Wq [N,K] s8 (host), *scale, bias [N] f32 (host). */
int kws_octbit_quantize(const float* W, int K, int N, int8_t* Wq, float* scale, float* bias);

/* Self-attention CTC model (models/attention_ctc.py:73-128 `inference`, DeployModel :215-274; config/attention_config.py),
 * batched over B independent utterances: each utterance's results are what the reference's batch-1 DeployModel gives for it,
 * whatever the other utterances and the padding.  Utterance b has T_b mel frames; c = combine_frame:
 *   stacking      c > 1: c - (T_b mod c) zero frames appended (1..c), rows of c frames -> T'_b = T_b / c + 1 rows of c*n_mel;
 *                 c == 1: T'_b = T_b (kws_attention_frames_out)
 *   embedding     x = row . W_in + b_in + pe[t'], pe[p][2i] = sin(p / 10000^(2i/H)), pe[p][2i+1] = cos(..), computed in double,
 *                 stored as float; the pad rows are real positions
 *   per layer     qkv = x . W_qkv + b_qkv; per head (d = hidden / num_heads) softmax(q k^T / sqrt(d)) v over the utterance's
 *                 T'_b keys, no mask, no output projection; y = LN_a(att + x); x = LN_b(relu(y . W1 + b1) . W2 + b2 + y)
 *   LN            tf.contrib.layers.layer_norm of TF 1.x: mean and population variance over the utterance's WHOLE [T'_b, H]
 *                 block, eps 1e-12, then * gamma + beta
 *   output        logits = relu?(x . W_out + b_out) (the post-relu logits: an extension, the reference graph exports only the
 *                 softmax), softmax over the classes
 * Supported (else KWS_ERR_UNSUPPORTED naming the field): n_mel * combine_frame <= 512, combine_frame 1..4, hidden 64/128/256
 * with hidden / num_heads 16 or 32, ffn_inner a multiple of 64 up to 1024, num_layers 1..8, num_classes 3..8, use_relu 0/1,
 * max_frames 1..8192 (the longest utterance a handle takes: the positional table holds max_frames / combine_frame + 1 rows).
 * Same conventions as a model handle: one host thread at a time per handle (KWS_ERR_BUSY), a call on another stream than the
 * previous one is ordered behind it by the handle's event, no device-wide wait except create, destroy and scratch growth. */
typedef struct kws_attention_config {
    int32_t n_mel;          /* F : mel bins per frame (config/attention_config.py:67: 60)       */
    int32_t combine_frame;  /* c : frames stacked per row (:79: 2)                               */
    int32_t hidden;         /* H : model width (:85: 128)                                         */
    int32_t num_heads;      /* multi_head_num (:84: 8)                                            */
    int32_t ffn_inner;      /* feed_forward_inner_size (:82: 512)                                 */
    int32_t num_layers;     /* L (:80: 3)                                                         */
    int32_t num_classes;    /* C (:88-91: 6)                                                      */
    int32_t use_relu;       /* relu on the logits (:55: 1)                                        */
    int32_t max_frames;     /* longest T_max a call may pass                                      */
} kws_attention_config;
typedef struct kws_attention* kws_attention_handle;
size_t kws_sizeof_attention_config(void);
/* Bytes of the canonical fp32 blob (0: invalid config), row-major, the 1x1 conv kernels squeezed to [in, out]:
 *   W_in [c*F, H]  b_in [H]
 *   per layer: W_qkv [H, 3H]  b_qkv [3H]  ln_a beta [H]  ln_a gamma [H]  W1 [H, Fi]  b1 [Fi]  W2 [Fi, H]  b2 [H]
 *              ln_b beta [H]  ln_b gamma [H]
 *   W_out [H, C]  b_out [C] */
size_t kws_attention_weights_nbytes(const kws_attention_config* cfg);
/* weights_blob: HOST memory of kws_attention_weights_nbytes(cfg) bytes.  With KWS_SELFTEST=1 the create runs
 * kws_attention_selftest and fails as it does. */
int kws_attention_create(const kws_attention_config* cfg, const void* weights_blob, size_t nbytes, kws_attention_handle* out);
/* ... with the precision of the matrix products: KWS_FP32 (exactly kws_attention_create) or KWS_F16X3 (the embedding, qkv and FFN
 * products on the fp16 matrix pipe, operands split into two fp16 pieces; same blob, same contract, same tolerance, NOT bit-identical
 * to KWS_FP32; activations, the attention core, layer norm, the output projection and softmax stay fp32).  KWS_BF16 / KWS_INT8:
 * KWS_ERR_UNSUPPORTED naming the precision.  KWS_F16X3 needs every W_in / W_qkv / W1 / W2 entry finite with |w| < 64, else
 * KWS_ERR_UNSUPPORTED naming the matrix, the layer and the value.  Precision and weights are validated before the device is probed. */
int kws_attention_create_precision(const kws_attention_config* cfg, int precision, const void* weights_blob, size_t nbytes,
                                   kws_attention_handle* out);
int kws_attention_destroy(kws_attention_handle h);   /* always KWS_OK */
/* T' of an utterance of T frames (>= 0), or a negative kws_status */
int kws_attention_frames_out(const kws_attention_config* cfg, int T);
/* Pre-sizes the scratch for calls of B utterances x T_max frames (the scratch only grows; growing synchronises once). */
int kws_attention_reserve(kws_attention_handle h, int B, int T_max);
/*   mel      [B, T_max, n_mel] f32 device
 *   lengths  [B] i32 device or NULL (= T_max): clamped to [0, T_max]; frames at or past T_b are never read into a result
 *   logits   [B, T'_max, C] f32 out or NULL; softmax [B, T'_max, C] f32 out or NULL (not both NULL); T'_max = frames_out(T_max)
 * Rows t' >= T'_b of both outputs are written as 0.  B == 0 or T'_max == 0 is a no-op. */
int kws_attention_run(kws_attention_handle h, const float* mel, const int32_t* lengths, int B, int T_max, float* logits,
                      float* softmax, void* stream);
/* Copies the fp32 positional table [max_frames / combine_frame + 1, hidden] (host memory) -- for inspection/tests. */
int kws_attention_pe_table(kws_attention_handle h, float* host_out);
/* Runs the handle's kernels on 3 random utterances (lengths T_max, T_max / 2 + 1 and 1) against a double-precision host loop
 * of the contract above; synchronises.  KWS_OK, or KWS_ERR_HIP with the deviation and kws_version(). */
int kws_attention_selftest(kws_attention_handle h);

/* The self-attention model on live streams: a sliding-window manager for B independent streams, ONE call per chunk and no host work
 * per stream.  The model carries no state, so "streaming" is what detector.py:158-209 does with its queue of softmax chunks, one stage
 * earlier: per stream a bounded FIFO of the last `window_chunks` chunks of MEL frames, cleared by the VAD on silence and by a trigger;
 * after every chunk the model runs over the concatenated window and ctc_decode2 + ctc_predict run over all of its output rows.  The
 * whole window is recomputed per chunk -- the positional table and the whole-block layer norm make every row depend on the window's
 * start and content, so nothing can be cached across chunks: a chunk costs one kws_attention_run over up to W frames per stream.
 * Arrival is per stream, as in kws_stream_feed_ragged: stream b reads the first n_b = n_per_stream[b] samples of row b of `pcm`
 * [B, n_max]; the lengths stay on the device (no host read, no host wait), are CLAMPED to [0, n_max], NULL means n_max for all;
 * n_max itself must lie in [0, max_chunk_samples].  Per feed and stream:
 *   n_b == 0                 the iteration is skipped: carry, window and chunk count stay bitwise as they are, hit[b] = 0, the stream
 *                            enters the model call with length 0 (an unchanged window that did not fire cannot fire)
 *   otherwise  VAD           vad(the n_b samples, vad_thres) false -> the window is emptied first                 (:168-177)
 *              front-end     mel of [carried samples | chunk], keep_b samples carried; carry_b + n_b < fft_size: every sample
 *                            is carried and the chunk completes zero frames                                      (:179-183)
 *              window        the chunk's frames (possibly none) take one slot; with window_chunks slots held the OLDEST slot is
 *                            dropped first with all of its frames (utils/queue.py:26-32, SimpleQueue.add)
 *              model         exactly kws_attention_run(window, lengths[b] = len_b frames, oldest first), frame stacking and zero pad
 *                            frames included
 *              decision      len_b == 0: no row is decoded, hit[b] = 0.  Otherwise ctc_decode2 (the first maximum over classes
 *                            1..C-2, strictly above decode_thres, repeats collapsed) over the T'_b = frames_out(len_b) rows and
 *                            hit[b] = `label` occurs in the decoded words (ctc_predict); on a hit the window is emptied (frames and
 *                            chunk count 0)
 *   softmax (or NULL)        [B, T'_max, C], T'_max = frames_out(W), W = window_chunks x frames(fft_size - 1 + max_chunk_samples):
 *                            what that kws_attention_run wrote, i.e. the rows the decision was taken on and zeros past T'_b (a
 *                            stream of length 0 has T'_b = 0 rows decoded; with combine_frame > 1 the model still writes its one
 *                            all-pad row)
 * A call with n_max == 0 skips every stream: hit and softmax are zeroed, nothing else is touched.
 * The handle BORROWS the attention and front-end handles (a call after either was destroyed: KWS_ERR_INVALID_ARGUMENT) and follows the
 * attention handle's rules: one host thread at a time (KWS_ERR_BUSY), a stream switch ordered by the handle's event.  It OWNS, per
 * stream, 2 x (fft_size - 1) carried samples and their lengths, the window of W x n_mel floats and window_chunks + 2 ints -- 86.1 KB
 * at the reference shape (n_mel 60, 15 chunks of 3600 samples: W = 15 x 23 = 345) -- and nothing else: one chunk's mel, the softmax, the gate's
 * masks and the model's lengths are carved out of a staging block of the ATTENTION handle that all its managers share; create also
 * reserves the model's scratch for (B, W), so a feed never allocates.  Both precisions of kws_attention_create_precision are served.
 * Launches per feed: front-end + gate, window update, the model's 2 + 3 L, decision = 5 + 3 L (kws_attention_stream_stats).
 * Refused before any device work, each naming the field: B < 1; window_chunks outside 1..64; a label that is empty, longer than 15
 * or with a digit outside 1..C-2; a null required pointer; handles that are not alive; a front-end that is not the magnitude-mel
 * 400-point FFT one (MFCC, power 2 and the dataset's framing are whole-utterance transforms; KWS_ERR_UNSUPPORTED); a front-end whose
 * n_mel differs from the model's; W greater than the model's max_frames (KWS_ERR_UNSUPPORTED). */
typedef struct kws_attention_stream* kws_attention_stream_handle;
int kws_attention_stream_create(kws_attention_handle model, kws_frontend_handle frontend, int B, int max_chunk_samples,
                                int window_chunks, float vad_thres, float decode_thres, const char* label,
                                kws_attention_stream_handle* out);
int kws_attention_stream_destroy(kws_attention_stream_handle h);   /* always KWS_OK */
int kws_attention_stream_feed(kws_attention_stream_handle h, const void* pcm /*[B,n_max] device*/, int n_max,
                              const int32_t* n_per_stream /*[B] device or NULL = n_max for all*/, int pcm_int16,
                              int32_t* hit /*[B] device*/, float* softmax /*[B,T'_max,C] device or NULL*/, void* stream);
/* Every stream b with slots[b] != 0 becomes what a fresh manager's stream is: carry length 0 and an empty window.  The other
 * streams stay bitwise untouched.  One launch. */
int kws_attention_stream_recycle(kws_attention_stream_handle h, const uint8_t* slots /*[B] device*/, void* stream);
/* Inspection, copies only, ordered like a feed: the windows as they stand -- mel [B, W, n_mel] (or NULL), the first frames[b] rows of
 * stream b oldest first (the rest is unspecified), and the slots held chunks[b] <= window_chunks. */
int kws_attention_stream_window(kws_attention_stream_handle h, float* mel /*[B,W,n_mel] device or NULL*/, int32_t* frames /*[B] device*/,
                                int32_t* chunks /*[B] device*/, void* stream);
/* The carried samples, as kws_stream_carry: samples [B, fft_size - 1], lengths [B], device. */
int kws_attention_stream_carry(kws_attention_stream_handle h, float* samples, int32_t* lengths, void* stream);
/* Bytes of device memory the handle owns, and the kernel launches of its last feed (0 after an n_max == 0 call); either may be NULL. */
int kws_attention_stream_stats(kws_attention_stream_handle h, size_t* device_bytes, int32_t* launches_last_feed);

/* Training of the self-attention CTC model (main.py --model attention; models/attention_ctc.py:131-202): taped forward, backward,
 * tf.nn.ctc_loss, tf.clip_by_global_norm, Adam / Nesterov.  fp32 only.
 *
 * What is trained is the function kws_attention_run serves, per utterance: stacking by combine_frame, embedding + positional table and
 * the L layers, each utterance over its own T'_b = frames_out(T_b) rows only -- attention over the utterance's own keys, layer-norm
 * moments over the utterance's own [T'_b, H] block (eps 1e-12).  This is the reference's training graph whenever all utterances of a
 * batch have the same length; on a padded batch the reference lets the padded rows take part as keys and in the layer-norm moments,
 * and this trainer does not (what is trained is what is served).  Rows at or past T'_b are never read into a result: NaN padding of x
 * gives the bits of zero padding.
 *
 * Training-only: dropout at the reference's three sites, each x * keep / keep_prob with a true division:
 *   site 0  the attention probabilities behind the softmax (:51-52; coordinates layer, b, head, row = query, col = key); the softmax's
 *           normaliser is the undropped sum
 *   site 1  the attention output in front of its residual sum (:106-108; head = 0, row = t', col = the unit 0..H-1)
 *   site 2  the FFN output in front of its residual sum (:114-116; as site 1)
 * The masks are no arrays: every keep decision is a stateless function of the call's drop_seed and (site, layer, b, head, row, col),
 *   ctr = site << 62 | layer << 58 | head << 52 | b << 28 | row << 14 | col
 *   z   = drop_seed + ctr * 0x9E3779B97F4A7C15                                       (all arithmetic modulo 2^64)
 *   z  ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *   keep iff (z >> 32) < floor((double)keep_prob * 2^32)
 * kws_attention_drop_keep evaluates it on the host for n (row, col) pairs: keep [n] bytes (0 / 1).  keep_prob == 1 ignores the seed and
 * gives the bits of a call without dropout.
 * Loss: tf.nn.ctc_loss on the (post-relu when use_relu) logits with sequence_length = T'_b, averaged as sum / B.  kws_train_grad's
 * conventions: blank is the last class; S_max <= 31; host seq_len (frames T_b, 0..T) / labels / label_len are range-checked before any
 * launch; an utterance without a valid path has loss +inf and a gradient of exactly 0; ctc_loss_kernel's LDS limit applies to T'.
 * Both relus (FFN inner, logits) use TensorFlow's ReluGrad, g * (pre > 0).  Clip, Adam and Nesterov exactly as kws_train_step; the
 * learning rate is an argument of every step.
 *
 * The entries are shaped after their kws_train_* namesakes: refusals come before the device is touched and name the field
 * (kws_attention_train_check decides them from host memory alone); the config space is kws_attention_create's; one host thread per
 * handle (KWS_ERR_BUSY); calls are ordered by the handle's event across streams; nothing allocates and nothing waits for the device
 * once the tape of a shape exists (kws_attention_train_reserve, or the first call of a larger shape) and the call's seq_len, labels and
 * label_len are those of the call before.  When they differ, the call uploads them (B * (3 + S_max) ints) from pageable host memory, as
 * kws_train_grad does: the runtime finishes that copy on the host before the call goes on, so the host waits for the stream's earlier
 * work once, and for nothing after it.
 *   x [B,T,n_mel] f32 device; seq_len [B], labels [B,S_max], label_len [B] host; loss [B] f32 device out
 *   grad_blob: device, kws_attention_weights_nbytes' layout, the gradient of sum(loss) / B; logits_or_null [B,T'max,C] device (rows past
 *   T'_b are 0); lr > 0; grad_norm_or_null: device, one float, the global norm before the clip
 *   set / get_weights, moments: the canonical blob in HOST memory; set zeroes the optimiser's slots and its step count
 *   stats: device bytes held; (re)allocations since create; optimiser steps since set_weights; kernel launches of the last grad / step
 *   call (12 + 19 L + use_relu, one more for a step); rows per chunk of the weight-gradient reduction */
typedef struct kws_attention_train_config {
    kws_attention_config model;
    int32_t optimizer;                /* KWS_OPT_ADAM / KWS_OPT_NESTEROV */
    float max_grad_norm;              /* <= 0: no clipping */
    float keep_prob;                  /* (0, 1] */
} kws_attention_train_config;
typedef struct kws_attention_train* kws_attention_train_handle;
size_t kws_sizeof_attention_train_config(void);
int kws_attention_train_create(const kws_attention_train_config* cfg, kws_attention_train_handle* out);
int kws_attention_train_check(const kws_attention_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels,
                              const int32_t* label_len, int B, int T, int S_max, const float* loss);
int kws_attention_train_destroy(kws_attention_train_handle h);   /* always KWS_OK */
int kws_attention_train_set_weights(kws_attention_train_handle h, const void* blob /*host*/, size_t nbytes, void* stream);
int kws_attention_train_get_weights(kws_attention_train_handle h, void* blob /*host*/, size_t nbytes, void* stream);
int kws_attention_train_reserve(kws_attention_train_handle h, int B, int T, int S_max);
int kws_attention_train_grad(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                             const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float* loss, float* grad_blob,
                             float* logits_or_null, void* stream);
int kws_attention_train_step(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                             const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float lr, float* loss,
                             float* grad_norm_or_null, void* stream);
int kws_attention_train_moments(kws_attention_train_handle h, float* m /*host*/, float* v /*host*/, void* stream);
int kws_attention_train_stats(kws_attention_train_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches,
                              int32_t* chunk_rows);
/* site 0..2, layer 0..7, b 0..65535, head 0..15, rows / cols [n] in 0..16383 (host); keep [n] bytes out (host) */
int kws_attention_drop_keep(uint64_t drop_seed, float keep_prob, int site, int layer, int b, int head, const int32_t* rows,
                            const int32_t* cols, int n, uint8_t* keep);

/* Frame-wise targets: the softmax cross-entropy of every frame against a class per frame (the reference README's frame-wise experiment,
 * "cross-entropy-like loss function ... the data need to be labeled to frame-wise"; the targets are what custom_keyword.frame_labels makes
 * of kws_ctc_align's path), as a whole-batch op and as the loss -- alone or mixed with the CTC loss -- of both train handles.
 *
 * For utterance b with n = seq_len[b], logits rows z_t of C classes (3..8), targets y_t in {-1, 0 .. C-1} (-1: no target for this frame;
 * the blank, class C-1, is a target like the others: frame_labels emits it) and class weights w_c >= 0, finite (NULL: all 1):
 *   W_b           = sum_{t<n, y_t>=0} w[y_t]
 *   ce_b          = (1 / W_b) sum_{t<n, y_t>=0} w[y_t] (logsumexp(z_t) - z_t[y_t])
 *   d ce_b / d z_t = (w[y_t] / W_b) (softmax(z_t) - e_{y_t}); exactly 0 at t >= n and at y_t = -1
 * i.e. torch.nn.functional.cross_entropy(z[:n], y[:n], weight=w, ignore_index=-1, reduction='mean') per utterance, except that W_b == 0
 * (an empty slot, no labelled frame, or only classes of weight 0) gives loss 0 and gradient 0 where torch gives NaN.  Frames
 * t >= seq_len[b] are never read, neither logits nor targets: NaN or garbage there gives the bits of zero padding.
 * targets is DEVICE memory ([B,T] int32; the attention handle: [B,T'], T' = kws_attention_frames_out(T)) and cannot be range-checked on
 * the host: a value outside [-1, C) at a live frame counts as -1, and that utterance's ce_b is reported as NaN -- loud, without an
 * out-of-bounds read and without a poisoned weight update.  seq_len and class_weight are HOST memory, checked before anything is
 * launched and shipped stream-ordered, as kws_ctc_loss ships its block.
 * One workgroup per utterance (an utterance's bits do not depend on its batch), fixed summation orders, no atomics: repeated calls
 * give the same bits.  No LDS per frame: no limit on T beyond B * T < 2^31.
 *
 *   kws_frame_loss   logits [B,T,C] f32 device -> loss [B] = ce_b and, unless NULL, grad_logits [B,T,C] (every row written).  Stateless,
 *                    stream-ordered, never synchronises, allocates only its host-to-device block.  Refused before the device is probed
 *                    (KWS_ERR_INVALID_ARGUMENT): B < 0, T < 1, C outside 3..8, B * T >= 2^31 (KWS_ERR_UNSUPPORTED), a NULL among logits /
 *                    seq_len / targets / loss, a pointer not 4-byte aligned, seq_len[b] outside [0,T], a weight negative or not finite.
 *
 * The train handles (plain, wrapped and carried-state alike; io_or_null as kws_train_grad_state's):
 *   loss[b] = ctc_weight ctc_b + frame_weight ce_b, and the gradient is that of J = sum_b loss[b] / B (plus <dstate_out, state_out>).
 *   ft->frame_loss, unless NULL, receives ce_b alone.  Between the logits product and the backward pass:
 *     ctc_weight == 0      one frame_loss launch (write mode, scale frame_weight / B): one launch fewer than the plain call.  labels and
 *                          label_len may be NULL and S_max is taken as 0; ctc_loss_kernel's LDS limit on T does not apply.
 *     both weights > 0     ctc_loss, train_scale with ctc_weight / B, then frame_loss adding onto the labelled rows: one launch more.
 *     frame_weight == 0    exactly the plain call's launches and bits; ctc_weight must then be 1 (a scaled CTC-only objective would
 *                          need a launch of its own for loss[b]; it is a learning-rate change) and ft->frame_loss is not written.
 *   The class weights travel in the handle's stream-ordered upload block behind the lengths and labels: the steady state allocates
 *   nothing and, with the lengths, labels and weights of the call before, uploads nothing.
 *   Refused before the device is touched: ft or ft->targets NULL; a weight (ctc, frame, class) negative or not finite; both of ctc_weight
 *   and frame_weight 0; frame_weight == 0 with ctc_weight != 1; targets or frame_loss not 4-byte aligned; everything the _state call
 *   refuses (with ctc_weight == 0 nothing about the labels).  kws_[attention_]train_check_frames decide all of it from host memory alone.
 *
 * The enrolment handle (kws_enroll_fit_frames): kws_enroll_fit with loss_trace[it,b] = ctc_weight ctc_b + frame_weight ce_b per step, ce_b
 * as above on the spliced rows logits2 over the C + n_new classes of the extended head -- targets [E*K,T] in ITS numbering: C-1 .. C+n_new-2
 * the new classes, C+n_new-1 the blank, what frame_labels(states, labels, blank = C+n_new-1) emits; class_weight [C + n_new].  Only the new
 * columns train: on column j the frame term's gradient at a labelled frame is frame_weight (w[y_t] / W_b) (softmax(z_t)[C-1+j] -
 * [y_t == C-1+j]) -- at a frame labelled with a trained class or the blank, the mass the new column has there.  The gradient of the
 * step's loss is summed over the K slots in slot order, divided by K, and goes through the unchanged Adam.  ft->frame_loss, unless
 * NULL, is [iterations, E*K] and receives ce_b alone at every step.
 *     ctc_weight == 0      one forward pass per step: project, softmax, accumulate.  No alpha / beta and no LDS per frame -- (3 + K)(H + 1)
 *                          n_new floats whatever T is, so kws_enroll_fit's limits on T and S_max do not apply (E * K * T < 2^31 does).
 *                          labels and label_len may be NULL, nothing about them is checked and S_max is taken as 0.
 *     both weights > 0     the frame term is accumulated in the forward pass (frames 0 .. n-1), the CTC term behind it in the beta pass
 *                          (frames n-1 .. 0); kws_enroll_fit's LDS.  A slot without a valid CTC path has loss +inf and a CTC gradient
 *                          of 0, and still contributes its frame term.
 *     frame_weight == 0    needs ctc_weight == 1: exactly kws_enroll_fit's launch and bits; ft->frame_loss is not written.
 *   W_b is computed once per launch (lane l of the slot's wave adds frames l, l + 64, .. in fp64, then a butterfly).  A target outside
 *   [-1, C + n_new) at a live frame counts as -1 and makes that slot's loss_trace and frame_loss NaN at every step; the update is that of
 *   -1 in its place, and nothing is read out of bounds.  The class weights ride in the handle's upload block behind [seq_len | label_len |
 *   labels]: with the ints and weights of the call before nothing is uploaded, the steady state allocates nothing, and kws_enroll_stats
 *   counts one allocation per shape.  The step count and the moments run on as kws_enroll_fit's do (N calls of one iteration give the
 *   bits of one call of N), and calls of the two entry points may be interleaved on one handle.
 *   Refused: everything above about ft (for C + n_new classes), everything kws_enroll_fit refuses (with ctc_weight == 0 nothing about
 *   the labels; LDS above 160 KiB with the byte counts in the mixed case only), E * K * T >= 2^31 (KWS_ERR_UNSUPPORTED).
 *   kws_enroll_check_frames decides all of it, and kws_enroll_create's refusals of the shape, from host memory alone.
 * Out of scope: label smoothing, targets in host memory, more than four slots per enrolment, training a frozen column. */
int kws_frame_loss(const float* logits /*device [B,T,C]*/, const int32_t* seq_len /*host [B]*/, const int32_t* targets /*device [B,T]*/,
                   const float* class_weight_or_null /*host [C]*/, int B, int T, int C, float* loss /*device [B]*/,
                   float* grad_logits_or_null /*device [B,T,C]*/, void* stream);
typedef struct kws_frame_targets {
    const int32_t* targets;       /* device [B,T] (attention: [B,T']) */
    const float*   class_weight;  /* host [C] or NULL */
    float          ctc_weight;    /* >= 0 */
    float          frame_weight;  /* >= 0 */
    float*         frame_loss;    /* device [B] out or NULL: ce_b alone */
} kws_frame_targets;
size_t kws_sizeof_frame_targets(void);
int kws_train_grad_frames(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                          int T, int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null,
                          const kws_train_state_io* io_or_null, const kws_frame_targets* ft, void* stream);
int kws_train_step_frames(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                          int T, int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null,
                          const kws_train_state_io* io_or_null, const kws_frame_targets* ft, void* stream);
int kws_train_check_frames(const kws_train_config* cfg, int wrapped, const float* x, const int32_t* seq_len, const int32_t* labels,
                           const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_train_state_io* io,
                           const kws_frame_targets* ft);
int kws_attention_train_grad_frames(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                                    const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float* loss, float* grad_blob,
                                    float* logits_or_null, const kws_frame_targets* ft, void* stream);
int kws_attention_train_step_frames(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                                    const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float lr, float* loss,
                                    float* grad_norm_or_null, const kws_frame_targets* ft, void* stream);
int kws_attention_train_check_frames(const kws_attention_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels,
                                     const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_frame_targets* ft);
int kws_enroll_fit_frames(kws_enroll_handle h, const float* nn_outputs, const float* logits1, const int32_t* seq_len,
                          const int32_t* labels_or_null, const int32_t* label_len_or_null, int T, int S_max, const kws_frame_targets* ft, float lr,
                          int iterations, float* loss_trace_or_null, void* stream);
int kws_enroll_check_frames(int H, int C, int n_new, int E, int K, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                            int T, int S_max, const kws_frame_targets* ft, float lr, int iterations);

#ifdef __cplusplus
}
#endif
#endif /* KWS_AMD_H_ */
