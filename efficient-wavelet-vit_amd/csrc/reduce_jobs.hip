// The host registry of the deferred weight-gradient reductions (reduce_jobs.h): a FIFO of jobs
// per (device, stream), and the kernel that runs what is still queued at a flush.
#include "reduce_jobs.h"

#include <deque>
#include <mutex>

namespace ewvit {

static thread_local bool t_defer_next = false;
static std::mutex g_red_mu;
static std::deque<std::pair<StreamKey, RedJob>> g_red_q;

bool reduce_take_defer() {
  const bool d = t_defer_next;
  t_defer_next = false;
  return d;
}

void reduce_defer(hipStream_t s, const RedJob &j) {
  std::lock_guard<std::mutex> lk(g_red_mu);
  g_red_q.emplace_back(stream_key(s), j);
}

RedJobs reduce_take_jobs(hipStream_t s) {
  RedJobs r;
  const StreamKey k = stream_key(s);
  std::lock_guard<std::mutex> lk(g_red_mu);
  int q = 0;
  for (auto it = g_red_q.begin(); it != g_red_q.end() && q < 2;) {
    if (it->first == k) {
      r.j[q] = it->second;
      r.j[q].nblk = red_job_blocks(it->second);
      r.nblk += r.j[q].nblk;
      ++q;
      it = g_red_q.erase(it);
    } else {
      ++it;
    }
  }
  r.nblk = (r.nblk + 7) / 8 * 8;
  return r;
}

// deferred jobs alone (ewvit_reduce_flush): 2 per launch
__global__ __launch_bounds__(256) void red_jobs_kernel(RedJobs rj) {
  __shared__ float red[256];
  run_red_jobs(rj, (int)blockIdx.x, red);
}

}  // namespace ewvit

using namespace ewvit;

extern "C" int ewvit_reduce_defer_next(int on) {
  t_defer_next = on != 0;
  return 0;
}

extern "C" int ewvit_reduce_pending(void *stream) {
  const StreamKey k = stream_key(as_stream(stream));
  std::lock_guard<std::mutex> lk(g_red_mu);
  int n = 0;
  for (auto &e : g_red_q)
    if (!stream || e.first == k) ++n;
  return n;
}

extern "C" int ewvit_reduce_flush(void *stream) {
  hipStream_t s = as_stream(stream);
  for (;;) {
    RedJobs rj = reduce_take_jobs(s);
    if (rj.nblk == 0) return 0;
    hipLaunchKernelGGL(red_jobs_kernel, dim3((unsigned)rj.nblk), dim3(256), 0, s, rj);
    if (int rc = launch_status("reduce_flush")) return rc;
  }
}
