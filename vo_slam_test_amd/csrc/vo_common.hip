// vo_common.hip -- error reporting, device bring-up and the process-wide options shared by every C-ABI entry point;
// the SE3 exp / log entry points.
#include "ba_math.h"
#include "vo_common.h"

#include <atomic>
#include <vector>

#include <mutex>

// process-wide developer knobs (vo_set_option)
static std::atomic<int> g_opt_ba_graph{0}, g_opt_pose_block{0}, g_opt_pairs_kernel{0}, g_opt_hamming_kernel{0};

namespace vo {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int ensure_device() {
  static std::once_flag once;
  static int status = VO_ERR_NO_DEVICE;
  std::call_once(once, [] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
      status = VO_ERR_NO_DEVICE;
      return;
    }
    status = VO_OK;
  });
  if (status != VO_OK)
    set_error("no usable HIP device: this library has no CPU fallback (build target gfx950 / MI355X)");
  return status;
}

static thread_local std::vector<DevBuf *> *g_scratch = nullptr;  // heap: no destructor order issues at thread exit
ScratchBuf::ScratchBuf() {
  if (!g_scratch) g_scratch = new std::vector<DevBuf *>();
  g_scratch->push_back(this);
}
size_t release_thread_scratch() {
  size_t freed = 0;
  if (g_scratch)
    for (DevBuf *b : *g_scratch) freed += b->bytes, b->release();
  return freed;
}

hipStream_t thread_stream() {
  thread_local hipStream_t st = nullptr;
  thread_local bool tried = false;
  if (!tried) {
    tried = true;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      st = nullptr;  // the NULL stream still gives correct results
    }
  }
  return st;
}

int copy_h2d(void *dst, const void *src, size_t bytes, hipStream_t st, const char *what) {
  if (!bytes) return VO_OK;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    set_error("%s: host-to-device copy of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    return VO_ERR_HIP;
  }
  return VO_OK;
}

int copy_d2h(void *dst, const void *src, size_t bytes, hipStream_t st, const char *what) {
  if (!bytes) return VO_OK;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) {
    set_error("%s: device-to-host copy of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    return VO_ERR_HIP;
  }
  return VO_OK;
}

int stream_sync(hipStream_t st, const char *what) {
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_error("%s: kernel or copy failed: %s", what, hipGetErrorString(e));
    return VO_ERR_HIP;
  }
  return VO_OK;
}

int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t st, const char *what) {
  VO_CHECK(b.reserve(bytes > 64 ? bytes : 64));
  return copy_h2d(b.p, src, bytes, st, what);
}

int opt_ba_graph() { return g_opt_ba_graph.load(std::memory_order_relaxed); }
int opt_pose_block() { return g_opt_pose_block.load(std::memory_order_relaxed); }
int opt_pairs_kernel() { return g_opt_pairs_kernel.load(std::memory_order_relaxed); }
int opt_hamming_kernel() { return g_opt_hamming_kernel.load(std::memory_order_relaxed); }

}  // namespace vo

using namespace vo::ba;  // vo_se3_exp / vo_se3_log

extern "C" {
const char *vo_last_error(void) { return vo::g_err; }
int vo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
const char *vo_version(void) { return "vo_slam_test_amd 0.1 (gfx950)"; }
size_t vo_release_thread_scratch(void) { return vo::release_thread_scratch(); }

int vo_set_option(int option, int value) {
  switch (option) {
    case VO_OPT_BA_GRAPH: g_opt_ba_graph.store(value != 0); return VO_OK;
    case VO_OPT_POSE_BLOCK:
      if (value != 0 && value != 64 && value != 128 && value != 256) {
        vo::set_error("vo_set_option(VO_OPT_POSE_BLOCK): 0 (automatic), 64, 128 or 256");
        return VO_ERR_INVALID;
      }
      g_opt_pose_block.store(value);
      return VO_OK;
    case VO_OPT_BA_PAIRS_KERNEL:
      if (value != 0 && value != 1) {
        vo::set_error("vo_set_option(VO_OPT_BA_PAIRS_KERNEL): 0 (blocks staged through LDS) or 1 (lane = couple, register loads)");
        return VO_ERR_INVALID;
      }
      g_opt_pairs_kernel.store(value);
      return VO_OK;
    case VO_OPT_HAMMING_KERNEL:
      if (value != 0 && value != 1) {
        vo::set_error("vo_set_option(VO_OPT_HAMMING_KERNEL): 0 (matrix cores) or 1 (VALU)");
        return VO_ERR_INVALID;
      }
      g_opt_hamming_kernel.store(value);
      return VO_OK;
    default: vo::set_error("vo_set_option: unknown option %d", option); return VO_ERR_INVALID;
  }
}

int vo_se3_exp(const double xi[6], double R[9], double t[3]) {
  if (!xi || !R || !t) return VO_ERR_INVALID;
  const Se3 T = se3_exp(xi);
  const double *q = T.q;
  const double tx = 2 * q[1], ty = 2 * q[2], tz = 2 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
  t[0] = T.t[0], t[1] = T.t[1], t[2] = T.t[2];
  return VO_OK;
}

int vo_se3_log(const double R[9], const double t[3], double xi[6]) {
  if (!xi || !R || !t) return VO_ERR_INVALID;
  se3_log_from_R(R, t, xi);  // (ba_math.h: shared with the device)
  return VO_OK;
}

}  // extern "C"
