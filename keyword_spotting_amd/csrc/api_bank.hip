// C ABI of libkws_amd.so (include/kws_amd.h): a bank of enrolled heads -- per-user customised keywords on one frozen model.  The
// handle (slots of new columns on the device), the utterance step and the stream manager whose head 2 comes from each stream's own
// slot.  The step itself is api_step.hip's (a heads step with HeadsArgs::bank set), the manager api_stream.hip's.
#include <new>

#include "api_internal.h"

using namespace kws_host;

namespace {

int bank_device_probe() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    return KWS_OK;
}

// the slot range of kws_bank_set / kws_bank_get
int bank_range(const kws_bank* bank, int first, int count, const void* Wn, const void* bn) {
    if (!bank) return fail(KWS_ERR_INVALID_ARGUMENT, "bank is null");
    if (!live_serial(bank)) return fail(KWS_ERR_INVALID_ARGUMENT, "the bank handle is not alive (destroyed, or not a handle)");
    if (first < 0 || count < 0 || (long long)first + count > bank->capacity)
        return fail(KWS_ERR_INVALID_ARGUMENT, "slots [%d, %d + %d) outside the bank's capacity %d", first, first, count, bank->capacity);
    if (count > 0 && (!Wn || !bn)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    return KWS_OK;
}

// slots [first, first + count) <-> caller buffers, stream-ordered
int bank_copy(kws_bank* bank, int first, int count, float* Wn, float* bn, bool set, void* stream) {
    KWS_TRY(bank_range(bank, first, count, Wn, bn));
    BusyGuard guard(bank->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this bank");
    if (count == 0) return KWS_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = (size_t)bank->H * bank->n_new, nw = (size_t)count * per * sizeof(float), nb = (size_t)count * bank->n_new * sizeof(float);
    float* W = bank->Wn + (size_t)first * per;
    float* b = bank->bn + (size_t)first * bank->n_new;
    KWS_HIP(hipMemcpyAsync(set ? W : Wn, set ? Wn : W, nw, hipMemcpyDeviceToDevice, st));
    KWS_HIP(hipMemcpyAsync(set ? b : bn, set ? bn : b, nb, hipMemcpyDeviceToDevice, st));
    return KWS_OK;
}

// what kws_step_bank, kws_step_bank_window and kws_stream_create_bank refuse about (model, bank, user) before anything else
int bank_args(const char* who, const kws_model* model, const kws_bank* bank, const int32_t* user) {
    if (!model) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!bank || !user) return fail(KWS_ERR_INVALID_ARGUMENT, "%s: bank or user is null", who);
    if (!live_serial(model)) return fail(KWS_ERR_INVALID_ARGUMENT, "model or window handle is not alive (destroyed, or not a handle)");
    return bank_serves(bank, model, who);
}

}  // namespace

int kws_host::bank_serves(const kws_bank* bank, const kws_model* h, const char* who) {
    if (!live_serial(bank)) return fail(KWS_ERR_INVALID_ARGUMENT, "the bank handle is not alive (destroyed, or not a handle)");
    if (h->num_classes2 <= 0)
        return fail(KWS_ERR_INVALID_ARGUMENT, "%s needs a model handle with a second class head (kws_create_heads): its plan and seams serve the bank", who);
    if (bank->H != h->cfg.hidden || bank->C != h->cfg.num_classes)
        return fail(KWS_ERR_INVALID_ARGUMENT, "the bank was created for hidden=%d C=%d, the model has hidden=%d C=%d", bank->H, bank->C, h->cfg.hidden,
                    h->cfg.num_classes);
    return KWS_OK;
}

const kws::BankSlotKeyword* kws_host::bank_slots(const kws_bank* bank) { return bank->keywords_ever ? bank->slots : nullptr; }

kws::BankRef kws_host::bank_ref(const kws_bank* bank, const int32_t* user) {
    kws::BankRef r = {};
    r.Wn = bank->Wn; r.bn = bank->bn; r.user = user; r.capacity = bank->capacity; r.n_new = bank->n_new;
    return r;
}

extern "C" {

int kws_bank_create(int H, int C, int n_new, int capacity, kws_bank_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (H != 64 && H != 128 && H != 256) return fail(KWS_ERR_UNSUPPORTED, "hidden=%d unsupported (64, 128, 256)", H);
    if (C < 3 || n_new < 1 || C + n_new > 8)
        return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d n_new=%d: the trained head has 3..7 classes and the extended one C + n_new <= 8", C, n_new);
    if (capacity < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "capacity=%d slots: at least one", capacity);
    KWS_TRY(bank_device_probe());
    kws_bank* h = new (std::nothrow) kws_bank();
    if (!h) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->H = H; h->C = C; h->n_new = n_new; h->capacity = capacity;
    const size_t nw = (size_t)capacity * H * n_new, nb = (size_t)capacity * n_new;
    const size_t floats = ((nw + nb) * sizeof(float) + 15) & ~(size_t)15;      // the slot table is read in 16-byte words
    // every slot starts without a keyword of its own: the manager's label2 over all n_new columns
    std::vector<kws::BankSlotKeyword> table((size_t)capacity);
    memset(table.data(), 0, table.size() * sizeof(kws::BankSlotKeyword));
    for (auto& s : table) s.n_used = n_new;
    h->keyword.assign((size_t)capacity, kws_bank::Keyword());
    for (auto& k : h->keyword) k.n_used = n_new;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->store), floats + table.size() * sizeof(kws::BankSlotKeyword));
    if (e == hipSuccess) e = hipMemset(h->store, 0, floats);
    if (e == hipSuccess)
        e = hipMemcpy(reinterpret_cast<char*>(h->store) + floats, table.data(), table.size() * sizeof(kws::BankSlotKeyword), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { kws_bank_destroy(h); return hip_fail(e, "kws_bank_create"); }
    h->Wn = h->store; h->bn = h->store + nw;
    h->slots = reinterpret_cast<kws::BankSlotKeyword*>(reinterpret_cast<char*>(h->store) + floats);
    live_register(h);
    *out = h;
    return KWS_OK;
}

int kws_bank_destroy(kws_bank_handle bank) {
    if (!bank) return KWS_OK;
    live_unregister(bank);
    hipDeviceSynchronize();
    if (bank->store) hipFree(bank->store);
    delete bank;
    return KWS_OK;
}

int kws_bank_set(kws_bank_handle bank, int first, int count, const float* Wn, const float* bn, void* stream) {
    return bank_copy(bank, first, count, const_cast<float*>(Wn), const_cast<float*>(bn), true, stream);
}

int kws_bank_get(kws_bank_handle bank, int first, int count, float* Wn, float* bn, void* stream) {
    return bank_copy(bank, first, count, Wn, bn, false, stream);
}

int kws_bank_set_keyword(kws_bank_handle bank, int slot, int n_used, const char* label, void* stream) {
    KWS_TRY(bank_range(bank, 0, 0, nullptr, nullptr));
    if (slot < 0 || slot >= bank->capacity) return fail(KWS_ERR_INVALID_ARGUMENT, "slot %d outside the bank's capacity %d", slot, bank->capacity);
    if (n_used < 1 || n_used > bank->n_new)
        return fail(KWS_ERR_INVALID_ARGUMENT, "n_used=%d: a slot's keyword uses 1..%d of the bank's new columns", n_used, bank->n_new);
    if (!label && n_used != bank->n_new)
        return fail(KWS_ERR_INVALID_ARGUMENT, "n_used=%d without a label: a slot without a keyword of its own has the bank's n_new=%d", n_used, bank->n_new);
    const int n = label ? (int)strnlen(label, 16) : 0;
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "a slot's label has up to 15 digits (the window's matcher has 16 states)");
    if (label) KWS_TRY(label_digits(label, n, nullptr));
    for (int i = 0; i < n; ++i)
        if (label[i] - '0' > bank->C + n_used - 2)
            return fail(KWS_ERR_INVALID_ARGUMENT, "label '%s': digit %c names a word class the slot's head does not have (C=%d, n_used=%d: words 1..%d)",
                        label, label[i], bank->C, n_used, bank->C + n_used - 2);
    BusyGuard guard(bank->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this bank");
    kws::BankSlotKeyword v;
    memset(&v, 0, sizeof(v));
    if (label) window_label_delta(label, n, v.delta);
    v.n_label = n; v.n_used = n_used; v.own = label ? 1 : 0;
    KWS_TRY(hip_done(kws::launch_bank_set_keyword(bank->slots + slot, v, static_cast<hipStream_t>(stream)), "launch bank_set_keyword"));
    kws_bank::Keyword& k = bank->keyword[(size_t)slot];
    k.n_used = n_used; k.own = label != nullptr;
    memset(k.label, 0, sizeof(k.label));
    if (label) memcpy(k.label, label, (size_t)n);
    if (label) bank->keywords_ever = true;
    return KWS_OK;
}

int kws_bank_get_keyword(kws_bank_handle bank, int slot, int* n_used, char* label, int* own) {
    KWS_TRY(bank_range(bank, 0, 0, nullptr, nullptr));
    if (slot < 0 || slot >= bank->capacity) return fail(KWS_ERR_INVALID_ARGUMENT, "slot %d outside the bank's capacity %d", slot, bank->capacity);
    BusyGuard guard(bank->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this bank");
    const kws_bank::Keyword& k = bank->keyword[(size_t)slot];
    if (n_used) *n_used = k.n_used;
    if (label) memcpy(label, k.label, sizeof(k.label));
    if (own) *own = k.own ? 1 : 0;
    return KWS_OK;
}

int kws_step_bank(kws_handle model, kws_bank_handle bank, const int32_t* user, const float* mel, const float* state_in, float* state_out,
                  const int32_t* seq_len, const uint8_t* reset_mask, float* nn_outputs, const kws_head_io* head1, const kws_head_io* head2, int B,
                  int T, void* stream) {
    KWS_TRY(bank_args("kws_step_bank", model, bank, user));
    BusyGuard guard(bank->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this bank");
    const kws::BankRef ref = bank_ref(bank, user);
    HeadsArgs ha;
    ha.nn_outputs = nn_outputs;
    ha.bank = &ref;
    ha.bank_slots = bank_slots(bank);
    if (head1) { ha.head[0] = *head1; ha.on[0] = true; }
    if (head2) { ha.head[1] = *head2; ha.on[1] = true; }
    StepArgs a;
    a.mel = mel; a.state_in = state_in; a.state_out = state_out; a.seq_len = seq_len; a.reset_mask = reset_mask;
    a.B = B; a.T = T; a.stream = static_cast<hipStream_t>(stream);
    a.heads = &ha;
    return step_impl(model, a);
}

int kws_stream_create_bank(kws_handle model, kws_frontend_handle frontend, kws_window_handle window1, kws_window_handle window2,
                           kws_bank_handle bank, const int32_t* user, int B, int max_chunk_samples, float vad_thres, const char* label1,
                           const char* label2, float* state, uint8_t* restart, kws_stream_handle* out) {
    if (out) *out = nullptr;
    if (!model || !window2 || !label2 || !bank || !user) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    KWS_TRY(bank_args("kws_stream_create_bank", model, bank, user));
    return stream_create_impl("kws_stream_create_bank", model, frontend, window1, window2, B, max_chunk_samples, vad_thres, label1, label2, state,
                              restart, out, bank, user);
}

int kws_step_bank_window(kws_handle h, kws_bank_handle bank, const int32_t* user, const float* mel, const float* state_in, float* state_out,
                         const uint8_t* reset_mask, int B, int T, kws_window_handle window1, kws_window_handle window2, const char* label1,
                         const char* label2, const uint8_t* clear_before, float* softmax1, float* softmax2, int32_t* hit, uint8_t* restart,
                         void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!bank || !user || !window1 || !window2 || !label1 || !label2 || !hit || !state_in || !state_out || (!mel && T > 0))
        return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (B < 1 || T < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d", B, T);
    if (!live_serial(window1) || !live_serial(window2))
        return fail(KWS_ERR_INVALID_ARGUMENT, "model or window handle is not alive (destroyed, or not a handle)");
    KWS_TRY(bank_args("kws_step_bank_window", h, bank, user));
    KWS_TRY(heads_window_check(h, window1, window2, B, T, bank));
    // rows of an even class count leave as float2 (store_row)
    if ((h->cfg.num_classes % 2 == 0 && (reinterpret_cast<uintptr_t>(softmax1) & 7) != 0) ||
        ((h->cfg.num_classes + bank->n_new) % 2 == 0 && (reinterpret_cast<uintptr_t>(softmax2) & 7) != 0))
        return fail(KWS_ERR_INVALID_ARGUMENT, "softmax1 / softmax2 must be 8-byte aligned");
    BusyGuard guard(bank->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this bank");
    KWS_TRY(window_bind_label(window1, label1));
    KWS_TRY(window_bind_label(window2, label2));
    const kws::BankRef ref = bank_ref(bank, user);
    HeadsArgs ha = heads_window_args(window1, window2, clear_before, hit, restart);
    ha.head[0].softmax = softmax1; ha.head[1].softmax = softmax2;
    ha.bank = &ref;
    ha.bank_slots = bank_slots(bank);
    StepArgs a;
    a.mel = mel; a.state_in = state_in; a.state_out = state_out; a.reset_mask = reset_mask;
    a.B = B; a.T = T; a.stream = static_cast<hipStream_t>(stream); a.heads = &ha;
    return step_impl(h, a);
}

}  // extern "C"
