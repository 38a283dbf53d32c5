// ABI bookkeeping of libscae_hip.so (see include/scae_hip.h).
#include "common.h"

#include <string.h>

#include <new>

extern "C" int scae_abi_version(void) { return SCAE_ABI_VERSION; }

extern "C" const char *scae_error_string(int code) {
  if (code == SCAE_OK) return "ok";
  if (code == SCAE_ERR_BAD_ARG) return "scae: null pointer or non-positive size";
  if (code == SCAE_ERR_UNSUPPORTED) return "scae: shape outside this build's kernel limits";
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "scae: unknown error";
}

// ---- launch lists (common.h: scae::launch) ------------------------------------------------
// The recordings that are open, each bound to ONE stream; a launch is appended to the
// recording of its own stream only.  This table is the bookkeeping of the handles the callers
// hold (like an allocator's), not state an entry point's result depends on.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

namespace {
struct Launch {
  const void *fn;
  dim3 grid, block;
  size_t lds;
  std::vector<unsigned long long> blob;   // the arguments, each at a 16-byte boundary
  std::vector<size_t> at;                 // byte offsets into blob (<= 64: common.h, launch_impl)
};
struct List {
  hipStream_t stream;
  bool open;
  std::vector<Launch> launches;
};
std::atomic<int> g_open{0};     // (scae::launch's fast path: nothing records)
std::mutex g_mu;                // (forward and backward launches come from different host threads)
std::vector<List *> g_lists;    // the open recordings
thread_local int t_launch_err = 0;

// the argument pointers hipLaunchKernel takes, into the launch's own copy of the bytes
void arg_ptrs(const Launch &l, void *ptrs[64]) {
  unsigned char *base =
      const_cast<unsigned char *>(reinterpret_cast<const unsigned char *>(l.blob.data()));
  for (size_t i = 0; i < l.at.size(); ++i) ptrs[i] = base + l.at[i];
}
bool is_open(const List *l) {
  std::lock_guard<std::mutex> lock(g_mu);
  return l->open;
}
}  // namespace

namespace scae_rec {
bool recording() { return g_open.load(std::memory_order_relaxed) > 0; }
void append(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, void *const *args,
            const size_t *sizes, int n) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (List *list : g_lists) {
    if (st != list->stream) continue;
    Launch l{fn, grid, block, lds, {}, {}};
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) {
      l.at.push_back(bytes);
      bytes += (sizes[i] + 15) & ~(size_t)15;
    }
    l.blob.assign((bytes + 7) / 8 + 2, 0ull);
    // (the vector's storage is 16-byte aligned by the allocator for these sizes)
    for (int i = 0; i < n; ++i)
      memcpy(reinterpret_cast<unsigned char *>(l.blob.data()) + l.at[i], args[i], sizes[i]);
    list->launches.push_back(std::move(l));
  }
}
// the hipError_t of the calling thread's first failed hipLaunchKernel (scae::launch), once
void note_launch_error(int e) {
  if (!t_launch_err) t_launch_err = e;   // (the first failure of a launcher that issues several)
}
int take_launch_error() {
  const int e = t_launch_err;
  t_launch_err = 0;
  return e;
}
}  // namespace scae_rec

static void close_list(List *l) {   // g_mu held
  if (!l->open) return;
  l->open = false;
  g_lists.erase(std::remove(g_lists.begin(), g_lists.end(), l), g_lists.end());
  g_open.fetch_sub(1);
}

extern "C" void *scae_launch_list_begin(void *stream) {
  List *l = new (std::nothrow) List{(hipStream_t)stream, true, {}};
  if (!l) return nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  g_lists.push_back(l);
  g_open.fetch_add(1);
  return l;
}
extern "C" int scae_launch_list_end(void *list) {
  SCAE_REQUIRE(list);
  std::lock_guard<std::mutex> lock(g_mu);
  List *l = static_cast<List *>(list);
  if (!l->open) return SCAE_ERR_BAD_ARG;
  close_list(l);
  return SCAE_OK;
}
extern "C" int scae_launch_list_size(const void *list) {
  if (!list) return 0;
  std::lock_guard<std::mutex> lock(g_mu);
  return (int)static_cast<const List *>(list)->launches.size();
}
// A closed list is immutable: a run or a timeline reads it without the lock.
extern "C" int scae_launch_list_run(const void *list, void *stream) {
  SCAE_REQUIRE(list);
  const List *ls = static_cast<const List *>(list);
  if (is_open(ls)) return SCAE_ERR_BAD_ARG;   // (still recording: it would record itself)
  for (const Launch &l : ls->launches) {
    void *ptrs[64];
    arg_ptrs(l, ptrs);
    hipError_t e = hipLaunchKernel(l.fn, l.grid, l.block, ptrs, l.lds, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  return SCAE_OK;
}
// One run of the list with a timing event in front of and behind every launch:
// out[2 i], out[2 i + 1] = start / end of launch i in microseconds after the first event -- the
// step's timeline as the device ran it.  Synchronises the stream; the event pairs add a few
// microseconds per launch.
extern "C" int scae_launch_list_timeline(const void *list, void *stream, void *side_stream,
                                         float *out_us, int n_out) {
  SCAE_REQUIRE(list && out_us);
  if (side_stream && side_stream != stream) return SCAE_ERR_BAD_ARG;
  const List *ls = static_cast<const List *>(list);
  if (is_open(ls)) return SCAE_ERR_BAD_ARG;
  const int n = (int)ls->launches.size();
  if (n_out < 2 * n) return SCAE_ERR_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  std::vector<hipEvent_t> ev;
  ev.reserve(2 * n);
  hipError_t rc = hipSuccess;
  for (int i = 0; rc == hipSuccess && i < 2 * n; ++i) {
    hipEvent_t e;
    rc = hipEventCreate(&e);
    if (rc == hipSuccess) ev.push_back(e);
  }
  for (int k = 0; rc == hipSuccess && k < n; ++k) {
    const Launch &l = ls->launches[k];
    void *ptrs[64];
    arg_ptrs(l, ptrs);
    rc = hipEventRecord(ev[2 * k], st);
    if (rc == hipSuccess) rc = hipLaunchKernel(l.fn, l.grid, l.block, ptrs, l.lds, st);
    if (rc == hipSuccess) rc = hipEventRecord(ev[2 * k + 1], st);
  }
  if (rc == hipSuccess) rc = hipStreamSynchronize(st);
  for (int i = 0; rc == hipSuccess && i < 2 * n; ++i) {
    float ms = 0.f;
    rc = hipEventElapsedTime(&ms, ev[0], ev[i]);
    out_us[i] = ms * 1e3f;
  }
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  return rc == hipSuccess ? SCAE_OK : (int)rc;
}
extern "C" int scae_launch_list_lane(const void *list, int i) {   // 0 for a launch, -1 past the end
  return i >= 0 && i < scae_launch_list_size(list) ? 0 : -1;
}
extern "C" void scae_launch_list_free(void *list) {
  if (!list) return;
  List *l = static_cast<List *>(list);
  {
    std::lock_guard<std::mutex> lock(g_mu);
    close_list(l);
  }
  delete l;
}
