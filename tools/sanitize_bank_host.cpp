// stand-alone CPU program: api_bank.hip's argument handling (every pre-device refusal and the device probe) under ASan + UBSan
#include <cstdio>
#include <cstring>
#include "kws_amd.h"
static int fails = 0;
#define EXPECT(call, code, text) do { int rc = (call); const char* e = kws_last_error(); \
    if (rc != (code) || (text[0] && !strstr(e, text))) { printf("FAIL %s -> %d '%s'\n", #call, rc, e); ++fails; } } while (0)
int main() {
    kws_bank_handle h = nullptr;
    float dummyf[4]; int32_t dummyi[4]; void* dummy = dummyf;
    EXPECT(kws_bank_create(128, 6, 2, 4, nullptr), KWS_ERR_INVALID_ARGUMENT, "out handle");
    EXPECT(kws_bank_create(100, 6, 2, 4, &h), KWS_ERR_UNSUPPORTED, "hidden=100");
    EXPECT(kws_bank_create(128, 6, 3, 4, &h), KWS_ERR_INVALID_ARGUMENT, "C=6 n_new=3");
    EXPECT(kws_bank_create(128, 2, 1, 4, &h), KWS_ERR_INVALID_ARGUMENT, "C=2");
    EXPECT(kws_bank_create(128, 6, 0, 4, &h), KWS_ERR_INVALID_ARGUMENT, "n_new=0");
    EXPECT(kws_bank_create(128, 6, 2, 0, &h), KWS_ERR_INVALID_ARGUMENT, "capacity=0");
    EXPECT(kws_bank_create(128, 6, 2, -5, &h), KWS_ERR_INVALID_ARGUMENT, "capacity=-5");
    EXPECT(kws_bank_create(128, 6, 2, 4, &h), KWS_ERR_NO_DEVICE, "no HIP device");
    EXPECT(kws_bank_destroy(nullptr), KWS_OK, "");
    EXPECT(kws_bank_set(nullptr, 0, 1, dummyf, dummyf, nullptr), KWS_ERR_INVALID_ARGUMENT, "bank is null");
    EXPECT(kws_bank_set((kws_bank_handle)dummy, 0, 1, dummyf, dummyf, nullptr), KWS_ERR_INVALID_ARGUMENT, "not alive");
    EXPECT(kws_bank_get((kws_bank_handle)dummy, 0, 1, dummyf, dummyf, nullptr), KWS_ERR_INVALID_ARGUMENT, "not alive");
    EXPECT(kws_bank_set_keyword(nullptr, 0, 1, "5", nullptr), KWS_ERR_INVALID_ARGUMENT, "bank is null");
    EXPECT(kws_bank_set_keyword((kws_bank_handle)dummy, 0, 1, "5", nullptr), KWS_ERR_INVALID_ARGUMENT, "not alive");
    EXPECT(kws_bank_set_keyword((kws_bank_handle)dummy, -1, 0, nullptr, nullptr), KWS_ERR_INVALID_ARGUMENT, "not alive");
    { int n = 0, own = 0; char label[16];
      EXPECT(kws_bank_get_keyword(nullptr, 0, &n, label, &own), KWS_ERR_INVALID_ARGUMENT, "bank is null");
      EXPECT(kws_bank_get_keyword((kws_bank_handle)dummy, 0, &n, label, &own), KWS_ERR_INVALID_ARGUMENT, "not alive"); }
    EXPECT(kws_step_bank(nullptr, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr),
           KWS_ERR_INVALID_ARGUMENT, "handle is null");
    EXPECT(kws_step_bank((kws_handle)dummy, nullptr, dummyi, dummyf, dummyf, dummyf, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr),
           KWS_ERR_INVALID_ARGUMENT, "bank or user is null");
    EXPECT(kws_step_bank((kws_handle)dummy, (kws_bank_handle)dummy, nullptr, dummyf, dummyf, dummyf, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr),
           KWS_ERR_INVALID_ARGUMENT, "bank or user is null");
    EXPECT(kws_step_bank((kws_handle)dummy, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr),
           KWS_ERR_INVALID_ARGUMENT, "not alive");
    kws_stream_handle out = (kws_stream_handle)dummy;
    uint8_t restart[4];
    EXPECT(kws_stream_create_bank((kws_handle)dummy, (kws_frontend_handle)dummy, (kws_window_handle)dummy, (kws_window_handle)dummy, nullptr, dummyi, 1, 3600,
                                  30.f, "12", "5", dummyf, restart, &out), KWS_ERR_INVALID_ARGUMENT, "null argument");
    if (out) { printf("FAIL out not cleared\n"); ++fails; }
    EXPECT(kws_stream_create_bank((kws_handle)dummy, (kws_frontend_handle)dummy, (kws_window_handle)dummy, (kws_window_handle)dummy, (kws_bank_handle)dummy,
                                  dummyi, 1, 3600, 30.f, "12", "5", dummyf, restart, &out), KWS_ERR_INVALID_ARGUMENT, "not alive");
    EXPECT(kws_stream_create_bank((kws_handle)dummy, (kws_frontend_handle)dummy, (kws_window_handle)dummy, (kws_window_handle)dummy, (kws_bank_handle)dummy,
                                  dummyi, 1, 3600, 30.f, "12", "5", dummyf, restart, nullptr), KWS_ERR_INVALID_ARGUMENT, "");
    EXPECT(kws_step_bank_window(nullptr, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, 1, 1, (kws_window_handle)dummy, (kws_window_handle)dummy,
                                "12", "5", nullptr, nullptr, nullptr, dummyi, nullptr, nullptr), KWS_ERR_INVALID_ARGUMENT, "handle is null");
    EXPECT(kws_step_bank_window((kws_handle)dummy, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, 0, 1, (kws_window_handle)dummy,
                                (kws_window_handle)dummy, "12", "5", nullptr, nullptr, nullptr, dummyi, nullptr, nullptr), KWS_ERR_INVALID_ARGUMENT, "bad shape");
    EXPECT(kws_step_bank_window((kws_handle)dummy, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, 1, 1, (kws_window_handle)dummy,
                                (kws_window_handle)dummy, "12", nullptr, nullptr, nullptr, nullptr, dummyi, nullptr, nullptr), KWS_ERR_INVALID_ARGUMENT, "null pointer");
    EXPECT(kws_step_bank_window((kws_handle)dummy, (kws_bank_handle)dummy, dummyi, dummyf, dummyf, dummyf, nullptr, 1, 1, (kws_window_handle)dummy,
                                (kws_window_handle)dummy, "12", "5", nullptr, nullptr, nullptr, dummyi, nullptr, nullptr), KWS_ERR_INVALID_ARGUMENT, "not alive");
    printf(fails ? "%d FAILED\n" : "all refusals as expected, %d failed\n", fails);
    return fails != 0;
}
