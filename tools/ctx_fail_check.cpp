// ctx_fail_check.cpp -- the context creators' failure path, for a leak-checked run without a device
// (tests/test_abi.py builds this with -fsanitize=address against libhrf.so and runs it with every
// HIP device hidden).  "leak" as the first argument loses one allocation on purpose, the test's
// proof that LeakSanitizer reports where it runs.
#include <cstdio>
#include <cstring>

#include "hrf.h"

static int check(const char *what, hrf_status st, const void *ctx) {
  const char *msg = hrf_last_error();
  if (st != HRF_EHIP || ctx || !msg || !msg[0]) {
    std::printf("%s: status %d, context %p, message '%s' (wanted HRF_EHIP, none, some)\n", what, (int)st, ctx,
                msg ? msg : "");
    return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "leak")) {
    volatile char *lost = new char[1920];
    lost[0] = 1;
    lost = nullptr;
    return 0;
  }
  int bad = 0;
  for (int i = 0; i < 3; ++i) {
    hrf_seg_ctx *seg = nullptr;
    bad += check("hrf_seg_ctx_create", hrf_seg_ctx_create(64, 64, &seg), seg);
    hrf_tile_ctx *tile = nullptr;
    bad += check("hrf_tile_ctx_create", hrf_tile_ctx_create(64, 64, &tile), tile);
  }
  if (hrf_live_allocations() != 0) {
    std::printf("hrf_live_allocations() = %lld after failed creates\n", (long long)hrf_live_allocations());
    ++bad;
  }
  if (hrf_seg_ctx_destroy(nullptr) != HRF_OK || hrf_tile_ctx_destroy(nullptr) != HRF_OK) {
    std::printf("destroy(NULL) failed\n");
    ++bad;
  }
  return bad ? 1 : 0;
}
