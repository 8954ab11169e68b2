// api.hip -- program runner and ABI introspection of libgode.so
#include "common.h"
#include "gif_lzw.h"

extern "C" int gode_version(void) { return GODE_VERSION; }

// host-side GIF LZW (gif_lzw.h): its error codes are GODE_E_ARG and GODE_E_SHAPE by value
static_assert((int)gif_lzw::ERR_ARG == (int)GODE_E_ARG && (int)gif_lzw::ERR_CAP == (int)GODE_E_SHAPE, "gif_lzw error codes");
extern "C" int64_t gode_gif_lzw_bound(int64_t n) { return gif_lzw::bound(n); }
extern "C" int64_t gode_gif_lzw(const uint8_t* idx, int64_t n, int32_t min_code_size, uint8_t* out, int64_t cap) {
  return gif_lzw::encode(idx, n, min_code_size, out, cap);
}

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

// ops [lo, hi) of a program on one stream.  Negative codes carry the op index: -(code*1000 + i).
static int run_range(const int32_t* kinds, const void* const* ops, int lo, int hi, void* stream) {
  for (int i = lo; i < hi; ++i) {
    int rc;
    switch (kinds[i]) {
#define GODE_RUN_ROW_(name, value, op_t, fn) case GODE_OP_##name: rc = fn((const op_t*)ops[i], stream); break;
      GODE_OPS(GODE_RUN_ROW_)
#undef GODE_RUN_ROW_
      case GODE_OP_PACK: {
        // every run of consecutive pack ops goes out as one launch per 8 panels
        int j = i;
        while (j + 1 < hi && kinds[j + 1] == GODE_OP_PACK) ++j;
        rc = gode_pack_batch_((const gode_pack_op* const*)(ops + i), j - i + 1, stream);
        if (rc == 0) i = j;
        break;
      }
      default: return GODE_E_KIND;
    }
    if (rc != 0) return rc > 0 ? rc : rc * 1000 - i;
  }
  return 0;
}

extern "C" int gode_run(const int32_t* kinds, const void* const* ops, int32_t n, void* stream) {
  if (n < 0 || (n > 0 && (!kinds || !ops))) return GODE_E_ARG;
  return run_range(kinds, ops, 0, n, stream);
}

// ---- two-lane runner ----------------------------------------------------------------------------------------------------
// The front of a program (ops that depend on nothing the previous program computed) runs on a side stream, so that it can
// sit under the tail of the previous program on the caller's stream.  The object owns the side stream and three events:
//   ev_entry    the caller's stream at entry (GODE_LANES_ORDERED: the side lane starts behind everything queued so far)
//   ev_front    the side lane behind its last op (the caller's stream waits for it before the first main op)
//   ev_release  the caller's stream behind op `release_after`: the last main op that touches a buffer the side lane writes
//               (GODE_LANES_OVERLAP: all the NEXT call's side lane waits for)
// An event wait takes the record that precedes it in host order, so one event of each kind serves every call.
struct gode_lanes {
  hipStream_t side;
  hipEvent_t ev_entry, ev_front, ev_release;
  bool released;      // ev_release holds the record of a call that went through: OVERLAP may wait for it
  bool entered;       // pair mode: ev_entry holds the record of a pair call's entry, a peer's OVERLAP may wait for it
};

#define GODE_HIP_TRY(expr)                          \
  do {                                              \
    hipError_t e__ = (expr);                        \
    if (e__ != hipSuccess) return (int)e__;         \
  } while (0)

extern "C" int gode_lanes_destroy(gode_lanes* l) {
  if (!l) return GODE_E_ARG;
  int rc = 0;
  if (l->side) {
    // queued work may still use the events' records: drain the lane before its objects go
    hipError_t e = hipStreamSynchronize(l->side);
    if (e != hipSuccess) rc = (int)e;
  }
  hipEvent_t evs[3] = {l->ev_entry, l->ev_front, l->ev_release};
  for (hipEvent_t ev : evs)
    if (ev) { hipError_t e = hipEventDestroy(ev); if (e != hipSuccess && rc == 0) rc = (int)e; }
  if (l->side) { hipError_t e = hipStreamDestroy(l->side); if (e != hipSuccess && rc == 0) rc = (int)e; }
  delete l;
  return rc;
}

extern "C" int gode_lanes_create(gode_lanes** out) {
  if (!out) return GODE_E_ARG;
  *out = nullptr;
  gode_lanes* l = new gode_lanes();      // (value-initialised: null handles, released = false)
  // non-blocking: a blocking stream synchronises implicitly with the legacy default stream, which is what the caller's
  // stream normally is -- the lanes would then run one after the other
  hipError_t e = hipStreamCreateWithFlags(&l->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&l->ev_entry, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&l->ev_front, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&l->ev_release, hipEventDisableTiming);
  // The runtime binds a stream to one of its few hardware queues at the stream's first command, to the least used one
  // at that moment.  Bind now, while the caller builds its plan, not at the first sampling call: by then a process may
  // have opened enough streams (a captured training iteration does) for the side stream to land on the caller's own
  // hardware queue, where the two lanes run one after the other.
  if (e == hipSuccess) e = hipEventRecord(l->ev_front, l->side);
  if (e != hipSuccess) {
    gode_lanes_destroy(l);
    return (int)e;
  }
  *out = l;
  return 0;
}

extern "C" void* gode_lanes_stream(gode_lanes* l) { return l ? (void*)l->side : nullptr; }

extern "C" int gode_run_lanes(gode_lanes* l, const int32_t* kinds, const void* const* ops, int32_t n, int32_t n_front,
                              int32_t release_after, int32_t mode, void* stream) {
  if (!l || n < 0 || (n > 0 && (!kinds || !ops)) || n_front < 0 || n_front > n || release_after < n_front ||
      release_after >= n || (mode != GODE_LANES_ORDERED && mode != GODE_LANES_OVERLAP))
    return GODE_E_ARG;
  hipStream_t main = (hipStream_t)stream;
  // A capturing stream takes the whole program in order: no fork inside a capture.  A query that fails (the legacy
  // stream while another stream captures) is answered the same way, and leaves no sticky error behind.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(main, &cap) != hipSuccess) {
    (void)hipGetLastError();
    cap = hipStreamCaptureStatusActive;
  }
  l->entered = false;                    // (ev_entry is about to hold something other than a pair call's entry)
  if (cap != hipStreamCaptureStatusNone) {
    l->released = false;
    return run_range(kinds, ops, 0, n, stream);
  }
  const bool overlap = mode == GODE_LANES_OVERLAP && l->released;
  l->released = false;                   // an error below leaves the next call ORDERED
  if (overlap) {
    GODE_HIP_TRY(hipStreamWaitEvent(l->side, l->ev_release, 0));
  } else {
    GODE_HIP_TRY(hipEventRecord(l->ev_entry, main));
    GODE_HIP_TRY(hipStreamWaitEvent(l->side, l->ev_entry, 0));
  }
  int rc = run_range(kinds, ops, 0, n_front, (void*)l->side);
  if (rc != 0) return rc;
  GODE_HIP_TRY(hipEventRecord(l->ev_front, l->side));
  GODE_HIP_TRY(hipStreamWaitEvent(main, l->ev_front, 0));
  rc = run_range(kinds, ops, n_front, release_after + 1, stream);
  if (rc != 0) return rc;
  GODE_HIP_TRY(hipEventRecord(l->ev_release, main));
  l->released = true;
  rc = run_range(kinds, ops, release_after + 1, n, stream);
  if (rc != 0) l->released = false;
  return rc;
}

// ---- pair mode: two whole programs in flight, on two lanes objects used in turn ---------------------------------------------
// Everything but the program's tail (its gode_bn_running op) runs on the object's own stream; the tail runs on the caller's
// stream behind the lane's last op.  Of the object's events, ev_entry is the caller's stream at this call's entry and ev_front
// the lane behind its last op.  The lane of call m waits for the entry event of call m-1 (the peer's): the programs of calls
// m-1 and m then run side by side, while everything the caller queued before call m-1 -- readers of result m-2, the tail of
// call m-2, both users of the buffers call m writes -- has run.
extern "C" int gode_run_pair(gode_lanes* l, gode_lanes* peer, const int32_t* kinds, const void* const* ops, int32_t n,
                             int32_t n_tail, int32_t mode, void* stream) {
  if (!l || peer == l || n < 2 || !kinds || !ops || n_tail < 1 || n_tail >= n ||
      (mode != GODE_LANES_ORDERED && mode != GODE_LANES_OVERLAP))
    return GODE_E_ARG;
  hipStream_t main = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(main, &cap) != hipSuccess) {
    (void)hipGetLastError();
    cap = hipStreamCaptureStatusActive;
  }
  l->released = false;                   // (a two-lane call on this object starts ORDERED)
  l->entered = false;                    // an error below leaves the peer's next call ORDERED
  if (cap != hipStreamCaptureStatusNone) return run_range(kinds, ops, 0, n, stream);
  const bool overlap = mode == GODE_LANES_OVERLAP && peer && peer->entered;
  GODE_HIP_TRY(hipEventRecord(l->ev_entry, main));
  GODE_HIP_TRY(hipStreamWaitEvent(l->side, overlap ? peer->ev_entry : l->ev_entry, 0));
  int rc = run_range(kinds, ops, 0, n - n_tail, (void*)l->side);
  // (also behind an op that failed: whatever the lane did take stays in front of the caller's next command)
  GODE_HIP_TRY(hipEventRecord(l->ev_front, l->side));
  GODE_HIP_TRY(hipStreamWaitEvent(main, l->ev_front, 0));
  if (rc != 0) return rc;
  rc = run_range(kinds, ops, n - n_tail, n, stream);
  if (rc != 0) return rc;
  l->entered = true;
  return 0;
}
