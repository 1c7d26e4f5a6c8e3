// Error plumbing and process state of the C-ABI (include/tpgan.h): the thread-local message of
// tpg_last_error(), the status helpers every entry point returns through (tpg_internal.h), the
// deterministic switch and the version string.
#include "tpg_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <string>

static thread_local std::string g_err;
static int g_det = 0;  // tpg_set_deterministic

int tpg::deterministic() { return __atomic_load_n(&g_det, __ATOMIC_RELAXED); }

int32_t tpg::fail(int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int32_t tpg::hip_check(int e, const char* what) {
  if (e == 0) return 0;
  return fail(e > 0 ? e : -100, "%s failed: %s", what, e > 0 ? hipGetErrorString((hipError_t)e) : "bad config");
}

int32_t tpg::launched(const char* what) { return hip_check((int)hipGetLastError(), what); }

extern "C" void tpg_set_deterministic(int32_t on) { __atomic_store_n(&g_det, on ? 1 : 0, __ATOMIC_RELAXED); }
extern "C" int32_t tpg_get_deterministic(void) { return tpg::deterministic(); }

extern "C" const char* tpg_version(void) { return "tpgan_hip 0.1 gfx950"; }
extern "C" const char* tpg_last_error(void) { return g_err.c_str(); }
