// The library's build identity (pmu_build_flags) and the debug build's violation records: every
// translation unit registers its PMU_DCHECK record here (pmu_common.h), pmu_debug_read / pmu_debug_reset
// walk the table.
#include "pmu_common.h"

#ifdef PMU_DEBUG
namespace {
struct DbgTu {
  const char* name;
  int (*rd)(int*);
  int (*rs)();
};
DbgTu g_dbg_tus[64];   // zero-initialised before any dynamic initialiser registers into it
int g_dbg_ntu = 0;
}  // namespace
int pmu_dbg_register(const char* tu, int (*rd)(int*), int (*rs)()) {
  if (g_dbg_ntu < 64) g_dbg_tus[g_dbg_ntu++] = DbgTu{tu, rd, rs};
  return g_dbg_ntu;
}
#endif

extern "C" int pmu_build_flags(void) {
  int f = 0;
#ifdef PMU_EXPERIMENTS
  f |= 1;
#endif
#ifdef PMU_DEBUG
  f |= 2;
#endif
  return f;
}

extern "C" int pmu_debug_read(int* out, const char** tu_name) {
  PMU_REQUIRE(out);
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (tu_name) *tu_name = nullptr;
#ifdef PMU_DEBUG
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;
  for (int t = 0; t < g_dbg_ntu; ++t) {
    int rec[4];
    const int rc = g_dbg_tus[t].rd(rec);
    if (rc) return rc;
    if (rec[3]) {
      for (int i = 0; i < 4; ++i) out[i] = rec[i];
      out[4] = t;
      if (tu_name) *tu_name = g_dbg_tus[t].name;
      return PMU_OK;
    }
  }
#endif
  return PMU_OK;
}

extern "C" int pmu_debug_reset(void) {
#ifdef PMU_DEBUG
  for (int t = 0; t < g_dbg_ntu; ++t) {
    const int rc = g_dbg_tus[t].rs();
    if (rc) return rc;
  }
#endif
  return PMU_OK;
}
