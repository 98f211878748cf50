// What the train handles share on the host (api_train_core.hip): the ordering of calls across HIP streams (the enrolment handle's too),
// the optimiser's state block, the arena that only grows, the job table of the weight-gradient launch, the update and the entry
// points that only touch the parameters.  A handle (api_train.hip, api_attention_train.hip) derives from TrainCore and adds its model.
#pragma once
#include <functional>

#include "api_internal.h"

#pragma GCC visibility push(hidden)
namespace kws_host {

// The ordering of a call against the handle's previous one: a call on another stream waits for `last_done` on the device.
struct CallOrder {
    hipStream_t last_stream = nullptr;
    bool valid = false;
    hipEvent_t last_done = nullptr;
    int enter(hipStream_t st);
    // ... at the end of a call's queued work, failed or not: launches that went out before a failure are still on `st`, and a following
    // call on another stream has to be ordered behind them.  rc: the call's result so far (its message stays the last error)
    int finish(hipStream_t st, int rc);
};

// the rows of the weight-gradient reduction are summed in at most kWgradMaxChunks chunks of a multiple of kWgradChunkUnit rows
constexpr int kWgradChunkUnit = 256, kWgradMaxChunks = 64;
inline int wgrad_chunk_rows(size_t rows) {
    const size_t per = (rows + (size_t)kWgradChunkUnit * kWgradMaxChunks - 1) / ((size_t)kWgradChunkUnit * kWgradMaxChunks);
    return (int)(kWgradChunkUnit * (per < 1 ? 1 : per));
}

// Lays an arena out in 256-byte aligned pieces.  base == null: only the size (`at` when done).
struct Carver {
    char* base;
    size_t at = 0;
    explicit Carver(char* b) : base(b) {}
    char* take(size_t bytes) { char* p = base ? base + at : nullptr; at += (bytes + 255) / 256 * 256; return p; }
    float* floats(size_t n) { return reinterpret_cast<float*>(take(n * sizeof(float))); }
};

struct TrainCore {
    int optimizer = KWS_OPT_ADAM;    // the config's
    float max_grad_norm = 0.f;
    size_t P = 0;                    // floats of the blob
    // one allocation fixed at create: theta | m | v | grad [4 P], the handle's own floats (`tail`), then the reduction's per-workgroup
    // sums of squares (doubles)
    float* state = nullptr;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr, *tail = nullptr;
    double* sumsq = nullptr;
    size_t state_bytes = 0;
    int nred = 0;
    // one allocation that only grows, carved by the handle for the shape of the call
    char* arena = nullptr;
    size_t arena_bytes = 0;
    std::vector<kws::TrainWgradJob> jobs_host;      // the products of the weight-gradient launch for the carved shape
    int units = 0;                   // ... and the work units of them all
    bool jobs_dirty = false;         // carved anew since the table last went to the device
    std::vector<int32_t> ints_host;  // the lengths and labels of the last call, as they are on the device
    int steps = 0, allocs = 0, launches = 0;
    std::atomic<int> in_call{0};
    CallOrder order;

    // one product of the weight-gradient launch, behind the ones before it (unit0)
    void add_job(int src, const float* a, int lda, int K, const float* d, int ldd, int N, size_t out, int ldo);
};

#define KWS_LAUNCH(h, call, what) do { KWS_TRY(hip_done((call), what)); ++(h)->launches; } while (0)

// the state block (tail_init: tail_floats host floats, or null for zeros) and the event; on a failure everything is released again and
// the result is the error of `who`
int train_core_create(TrainCore* c, size_t P, size_t tail_floats, const float* tail_init, const char* who);
void train_core_destroy(TrainCore* c);
// an arena of `need` bytes: grown if it has to be (waits for the device once; the arena is null if that fails).  Empties the job table
// and forgets the ints: the caller carves and builds its jobs next
int train_arena_reserve(TrainCore* c, size_t need, int B, int T, int layers);
// the job table, once per carve, and the call's packed ints when they differ from the last call's
int train_upload(TrainCore* c, kws::TrainWgradJob* d_jobs, int32_t* d_ints, std::vector<int32_t>* ints, hipStream_t st);
// clip over c->grad (its blocks' sums of squares in c->sumsq), one optimiser step with the moments and the step count
int train_update(TrainCore* c, float lr, float* grad_norm_or_null, hipStream_t st);
// one host thread at a time, ordered behind the previous call, `body` on the stream; sync: the host then waits for the stream
int train_call(TrainCore* c, void* stream, const std::function<int(hipStream_t)>& body, bool sync = false);
// the bodies of kws_*train_set_weights (then: what follows the copy inside the call, or null), _get_weights, _moments and _stats
int train_set_weights(TrainCore* c, const void* blob, size_t nbytes, void* stream, const std::function<int(hipStream_t)>& then);
int train_get_weights(TrainCore* c, void* blob, size_t nbytes, void* stream);
int train_moments(TrainCore* c, float* m, float* v, void* stream);
int train_stats(const TrainCore* c, int cv_chunk_rows, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches, int32_t* chunk_rows);
// the refusals both create functions share, and of the CTC loss over `rows` rows: S_max, and the LDS of ctc_loss_kernel
int check_optimizer(float keep_prob, int optimizer, float max_grad_norm);
int check_s_max(int S_max);
int check_ctc_lds(int rows, int S_max, const char* rows_text);

}  // namespace kws_host
#pragma GCC visibility pop
