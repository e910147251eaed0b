// lotus-hip: C-ABI plumbing shared by every op family (error string, version).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static thread_local char g_err[512] = "";
__attribute__((visibility("hidden"))) __thread hipEvent_t lotus_tls_stop_event = nullptr;  // see LOTUS_LAUNCH (common.h)

// route of the calling thread's last dense product (gemm_common.h: lotus_note_dense_route; read by lotus_dense_last_route)
__attribute__((visibility("hidden"))) __thread int lotus_tls_dense_route[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// route of the calling thread's last sparse-convolution launch (conv_route.h; read by lotus_conv_last_route)
__attribute__((visibility("hidden"))) __thread int lotus_tls_conv_route[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// route of the calling thread's last attention launch (attn_route.h; read by lotus_attention_last_route)
__attribute__((visibility("hidden"))) __thread int lotus_tls_attn_route[8] = {0, 0, 0, 0, 0, 0, 0, 0};

void lotus_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {
const char* lotus_last_error(void) { return g_err; }
// 2 (round 5): lotus_subm_conv / lotus_cpe_fwd / _bwd take a tap plan, lotus_adamw_step takes double betas + shadow pointers,
// lotus_fe_neighbours needs 16-byte hash slots, the counter buffer grew by the BatchNorm counters (all round 4)
int lotus_abi_version(void) { return 3; }

// Stream link: a caller-owned ring of timing-less events used to order one stream after another without a host
// round trip ("to" waits for everything enqueued on "from" so far, or — lotus_link_next_event — for one launch).  Re-recording a ring event later is safe:
// hipStreamWaitEvent captures the event's state at the time of the call.
struct StreamLink {
  int n, next;
  hipEvent_t ev[1];
};
unsigned long long lotus_streamlink_create(int nevents) {
  if (nevents < 1 || nevents > 4096) {
    lotus_set_error("lotus_streamlink_create: nevents out of range");
    return 0;
  }
  StreamLink* l = (StreamLink*)malloc(sizeof(StreamLink) + sizeof(hipEvent_t) * (nevents - 1));
  if (!l) return 0;
  l->n = nevents;
  l->next = 0;
  for (int i = 0; i < nevents; ++i) {
    // Device-side ordering only (hipStreamWaitEvent / stop events; never inspected from the host), so the system-scope
    // fence a recorded event performs by default is dropped: kernels of one device synchronise through their own
    // agent-scope acquire / release.  Measured +0.5-1.3 % step throughput.
    hipError_t e = hipEventCreateWithFlags(&l->ev[i], hipEventDisableTiming | hipEventDisableSystemFence);
    if (e != hipSuccess) {
      lotus_set_error("lotus_streamlink_create: %s", hipGetErrorString(e));
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(l->ev[j]);
      free(l);
      return 0;
    }
  }
  return (unsigned long long)(uintptr_t)l;
}
int lotus_streamlink_wait(unsigned long long link, void* from_stream, void* to_stream) {
  StreamLink* l = (StreamLink*)(uintptr_t)link;
  if (!l) {
    lotus_set_error("lotus_streamlink_wait: null link");
    return -1;
  }
  hipEvent_t ev = l->ev[l->next];
  l->next = (l->next + 1) % l->n;
  hipError_t e = hipEventRecord(ev, (hipStream_t)from_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)to_stream, ev, 0);
  if (e != hipSuccess) {
    lotus_set_error("lotus_streamlink_wait: %s", hipGetErrorString(e));
    return -2; /* LOTUS_E_LAUNCH */
  }
  return 0;
}
}  // extern "C"
// internal (blocks.cpp): the ring's next event, to be bound to a kernel launch as its stop event
hipEvent_t lotus_link_next_event(unsigned long long link) {
  StreamLink* l = (StreamLink*)(uintptr_t)link;
  if (!l) return nullptr;
  hipEvent_t ev = l->ev[l->next];
  l->next = (l->next + 1) % l->n;
  return ev;
}
extern "C" {
int lotus_streamlink_destroy(unsigned long long link) {
  StreamLink* l = (StreamLink*)(uintptr_t)link;
  if (!l) return 0;
  for (int i = 0; i < l->n; ++i) (void)hipEventDestroy(l->ev[i]);
  free(l);
  return 0;
}
}
