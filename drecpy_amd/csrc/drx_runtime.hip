// Library bookkeeping of libdrx.so: version, error strings, the host's copy of the mask hash, light events and streams.  No kernels.
#include "drx_common.hpp"

using namespace drx;

extern "C" {

int drx_version(void) { return DRX_VERSION; }

const char *drx_strerror(int code) {
  switch (code) {
    case DRX_OK: return "ok";
    case DRX_EINVAL: return "invalid argument";
    case DRX_ESCRATCH: return "scratch buffer too small";
    case DRX_ENOTIMPL: return "not implemented";
    case DRX_ERETRY: return "sampler gave up after its maximum number of consecutive failed attempts";
    case DRX_ECOMM: return "RCCL transport error (drx_comm_last_error() has the text)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown drx error";
  }
}

uint32_t drx_hash_u32(uint64_t seed, uint32_t a, uint32_t b) { return hash_u32(seed, a, b); }

// ---- light events for the run-ahead pipelines: ordering between two streams of ONE device.  hipEventDisableSystemFence: the record
// releases at agent scope instead of writing the L2 back for the host and peers — all a same-device hipStreamWaitEvent needs.
void *drx_event_create(void) {
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return (void *)e;
}
void drx_event_destroy(void *ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
int drx_event_record(void *ev, void *stream) { return ev ? (int)hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) : DRX_EINVAL; }
int drx_stream_wait_event(void *stream, void *ev) { return ev ? (int)hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0) : DRX_EINVAL; }
int drx_event_synchronize(void *ev) { return ev ? (int)hipEventSynchronize((hipEvent_t)ev) : DRX_EINVAL; }

void *drx_stream_create_cu_slice(int32_t cus_per_xcd) {
  constexpr int kXcds = 8, kCusPerXcd = 32;          // gfx950
  if (cus_per_xcd < 1 || cus_per_xcd > kCusPerXcd) return nullptr;
  uint32_t mask[kXcds * kCusPerXcd / 32] = {};
  for (int c = kCusPerXcd - cus_per_xcd; c < kCusPerXcd; ++c)
    for (int x = 0; x < kXcds; ++x) {
      const int bit = c * kXcds + x;
      mask[bit >> 5] |= 1u << (bit & 31);
    }
  hipStream_t st = nullptr;
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)(sizeof(mask) / sizeof(mask[0])), mask) != hipSuccess) return nullptr;
  return (void *)st;
}
void drx_stream_destroy(void *stream) { if (stream) (void)hipStreamDestroy((hipStream_t)stream); }

}  // extern "C"
