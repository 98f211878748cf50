// stand-alone CPU program: api_beam.hip's argument handling (every pre-device refusal and the device probe) under ASan + UBSan
#include <cstdio>
#include <cstring>
#include "kws_amd.h"
static int fails = 0;
#define EXPECT(call, code, text) do { int rc = (call); const char* e = kws_last_error(); \
    if (rc != (code) || (text[0] && !strstr(e, text))) { printf("FAIL %s -> %d '%s'\n", #call, rc, e); ++fails; } } while (0)
int main() {
    alignas(16) float x[8];
    int32_t p[8], n[8], s[8];
    float lp[8];
    const int bad = KWS_ERR_INVALID_ARGUMENT;
    EXPECT(kws_ctc_beam_search(nullptr, s, 1, 1, 6, 5, 1, 8, 1, p, n, lp, nullptr), bad, "null pointer");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 8, 1, nullptr, n, lp, nullptr), bad, "null pointer");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 8, 1, p, nullptr, lp, nullptr), bad, "null pointer");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 8, 1, p, n, nullptr, nullptr), bad, "null pointer");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 2, 5, 1, 8, 1, p, n, lp, nullptr), bad, "C=2");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 9, 5, 1, 8, 1, p, n, lp, nullptr), bad, "C=9");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 0, 1, 8, 1, p, n, lp, nullptr), bad, "beam_width=0");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 33, 1, 8, 1, p, n, lp, nullptr), bad, "beam_width=33");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 0, 8, 1, p, n, lp, nullptr), bad, "top_paths=0");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 6, 8, 1, p, n, lp, nullptr), bad, "top_paths=6");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 0, 1, p, n, lp, nullptr), bad, "L_max=0");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 65, 1, p, n, lp, nullptr), bad, "L_max=65");
    EXPECT(kws_ctc_beam_search(x, s, 0, 1, 6, 5, 1, 8, 1, p, n, lp, nullptr), bad, "B=0");
    EXPECT(kws_ctc_beam_search(x, s, 1, -2, 6, 5, 1, 8, 1, p, n, lp, nullptr), bad, "T=-2");
    EXPECT(kws_ctc_beam_search(x + 1, s, 1, 1, 6, 5, 1, 8, 1, p, n, lp, nullptr), bad, "16-byte aligned");
    EXPECT(kws_ctc_beam_search(x, s, 1, 1, 6, 5, 1, 8, 1, p, n, reinterpret_cast<float*>(reinterpret_cast<char*>(lp) + 1), nullptr), bad, "4-byte aligned");
    EXPECT(kws_ctc_beam_search(x, s, 1, 4885, 6, 5, 1, 8, 1, p, n, lp, nullptr), KWS_ERR_UNSUPPORTED, "163872 bytes exceed the 163840");
    EXPECT(kws_ctc_beam_search(x, s, 1, 2147483647, 6, 5, 1, 8, 1, p, n, lp, nullptr), KWS_ERR_UNSUPPORTED, "exceed");
    EXPECT(kws_ctc_beam_search(x, nullptr, 1, 1, 6, 5, 1, 8, 0, p, n, lp, nullptr), KWS_ERR_NO_DEVICE, "no HIP device");
    EXPECT(kws_ctc_beam_search(x, s, 2147483647, 4884, 8, 32, 32, 64, 1, p, n, lp, nullptr), KWS_ERR_NO_DEVICE, "no HIP device");
    printf(fails ? "%d FAILED\n" : "all refusals as expected, %d failed\n", fails);
    return fails != 0;
}
