// api.hip -- program runner and ABI introspection of libgode.so
#include "common.h"

extern "C" int gode_version(void) { return GODE_VERSION; }

extern "C" int gode_sizeof(int kind) {
  switch (kind) {
    case 0: return (int)sizeof(gode_conv_geom);
    case -1: return (int)sizeof(gode_adam_noise_tensor);
    case GODE_OP_PACK: return (int)sizeof(gode_pack_op);
#define GODE_SIZEOF_ROW_(name, value, op_t, fn) case GODE_OP_##name: return (int)sizeof(op_t);
    GODE_OPS(GODE_SIZEOF_ROW_)
#undef GODE_SIZEOF_ROW_
  }
  return GODE_E_KIND;
}

// Executes a pre-built list of ops back to back on one stream: one host->library call per network pass keeps the
// launch path short at batch 32, where a whole generator forward is ~1 ms of GPU time.
extern "C" int gode_pack_batch_(const gode_pack_op* const* ops, int n, void* stream);   // igemm.hip

extern "C" int gode_run(const int32_t* kinds, const void* const* ops, int32_t n, void* stream) {
  if (n < 0 || (n > 0 && (!kinds || !ops))) return GODE_E_ARG;
  for (int i = 0; i < n; ++i) {
    int rc;
    switch (kinds[i]) {
#define GODE_RUN_ROW_(name, value, op_t, fn) case GODE_OP_##name: rc = fn((const op_t*)ops[i], stream); break;
      GODE_OPS(GODE_RUN_ROW_)
#undef GODE_RUN_ROW_
      case GODE_OP_PACK: {
        // every run of consecutive pack ops goes out as one launch per 8 panels
        int j = i;
        while (j + 1 < n && kinds[j + 1] == GODE_OP_PACK) ++j;
        rc = gode_pack_batch_((const gode_pack_op* const*)(ops + i), j - i + 1, stream);
        if (rc == 0) i = j;
        break;
      }
      default: return GODE_E_KIND;
    }
    if (rc != 0) return rc > 0 ? rc : rc * 1000 - i;  // negative codes carry the op index: -(code*1000 + i)
  }
  return 0;
}
