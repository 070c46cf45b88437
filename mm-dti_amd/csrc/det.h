// Deterministic mode, host side: the process-wide flag, the per-stream table of reduction workspaces, and the sizes the fixed-order
// forms need -- plain host C++17 (no HIP types), so that tests/det_table_main.cpp can run it under a host sanitizer without a GPU.
//
// With the flag on, a launcher whose default form lets workgroups meet in fp32 atomics stores per-workgroup partials into the workspace
// registered for ITS launch stream and folds them in a fixed order with a kernel queued directly behind on the same stream.  Kernels of
// one stream run in order, so one workspace per stream is race-free.  The table is read on the host, in the launchers, never on the device.
#pragma once
#include <atomic>
#include <mutex>
#include <vector>

#include "stream_plan.h"

namespace mmdti {

struct DetSlot {
  void* stream;
  void* ws;
  long long bytes;
};

class DetTable {
 public:
  void set_on(bool on) { on_.store(on, std::memory_order_relaxed); }
  bool on() const { return on_.load(std::memory_order_relaxed); }     // (every launcher asks, in the default mode too: no lock)
  // ws != null: registers (or replaces) the stream's workspace; ws == null: forgets it.  false: ws without bytes, or not 16-byte aligned
  bool put(void* stream, void* ws, long long bytes) {
    std::lock_guard<std::mutex> g(mu_);
    size_t i = 0;
    while (i < slots_.size() && slots_[i].stream != stream) ++i;
    if (!ws) {
      if (i < slots_.size()) slots_.erase(slots_.begin() + (long)i);
      return true;
    }
    if (bytes <= 0 || (reinterpret_cast<unsigned long long>(ws) & 15ull) != 0) return false;
    if (i < slots_.size()) slots_[i] = DetSlot{stream, ws, bytes};
    else slots_.push_back(DetSlot{stream, ws, bytes});
    return true;
  }
  bool get(void* stream, DetSlot* out) const {
    std::lock_guard<std::mutex> g(mu_);
    for (const DetSlot& s : slots_)
      if (s.stream == stream) {
        *out = s;
        return true;
      }
    return false;
  }
  size_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return slots_.size();
  }

 private:
  mutable std::mutex mu_;
  std::atomic<bool> on_{false};
  std::vector<DetSlot> slots_;
};
inline DetTable& det_table() {
  static DetTable t;
  return t;
}

// ---- launch geometry the workspace sizes follow from (the launchers use the same functions: ln_bwd_grid of row_plan.h, colsum_grid_y
// of stream_plan.h) ----
static inline int det_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// unfused pair-bias feature backward in the mode: workgroups (16 pairs per iteration each)
static inline int gbf_features_bwd_grid(long long P) {
  const long long b = (P + 15) / 16;
  return (int)(b > 256 ? 256 : (b < 1 ? 1 : b));
}

// bytes of workspace one launch of a site needs (MMDTI_DET_* of mmdti_hip.h); -1: unknown site or bad shape
static inline long long det_workspace_bytes(int site, long long rows, long long cols) {
  if (rows <= 0 || cols <= 0) return -1;
  switch (site) {
    case 1: return rows > 0x7fffffffLL || cols > 2048 ? -1 : (long long)ln_bwd_grid((int)rows, (int)cols) * 3 * cols * 4;  // [wg][3][D]
    case 2: return rows > 0x7fffffffLL ? -1 : (long long)colsum_grid_y((int)rows) * cols * 4;                              // [gy][cols]
    case 3: return rows * cols * 4;                                                                                      // one [M][N] slab
    case 4: return (long long)gbf_features_bwd_grid(rows) * cols * 4;                                                    // [wg][2 E + 2 K], rows = pairs
    default: return -1;
  }
}

// Split-K in the mode: the partial tiles go to slabs of the stream's workspace.  The most splits (<= the requested count) whose slabs fit,
// renormalised so that no split is empty (the slab pass sums EVERY slab); 1 when not even two fit -- one split is always deterministic.
static inline int det_fit_splits(int splitk, int ktiles, long long slab_elems, long long ws_bytes) {
  if (splitk < 1) splitk = 1;
  if (ktiles < 1) ktiles = 1;
  long long fit = slab_elems > 0 ? ws_bytes / (slab_elems * 4) : 0;
  int sk = fit < splitk ? (int)fit : splitk;
  if (sk > ktiles) sk = ktiles;
  if (sk < 2) return 1;
  return det_cdiv(ktiles, det_cdiv(ktiles, sk));
}

}  // namespace mmdti
