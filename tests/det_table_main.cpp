// Stand-alone host program over mm-dti_amd/csrc/det.h (the deterministic mode's flag, per-stream workspace table, workspace sizes and
// split rule).  No GPU, no HIP: tests/test_deterministic_cpu.py builds it with -fsanitize=address,undefined and runs it.
// Prints "ok" and exits 0, or prints the failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../mm-dti_amd/csrc/det.h"

using namespace mmdti;

static int fails = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                 \
    }                                                          \
  } while (0)

int main() {
  DetTable t;
  DetSlot s;
  CHECK(!t.on());
  t.set_on(true);
  CHECK(t.on());
  t.set_on(false);
  CHECK(!t.on());

  // register, replace, look up, forget -- the null stream is a key like any other
  alignas(16) static char a[64], b[64];
  void* s0 = nullptr;
  void* s1 = reinterpret_cast<void*>(0x1000);
  CHECK(!t.get(s0, &s));
  CHECK(t.put(s0, a, 64));
  CHECK(t.put(s1, b, 32));
  CHECK(t.size() == 2);
  CHECK(t.get(s0, &s) && s.ws == a && s.bytes == 64);
  CHECK(t.get(s1, &s) && s.ws == b && s.bytes == 32);
  CHECK(t.put(s0, b, 48));                  // replace
  CHECK(t.size() == 2);
  CHECK(t.get(s0, &s) && s.ws == b && s.bytes == 48);
  CHECK(!t.put(s1, a + 4, 16));             // misaligned
  CHECK(!t.put(s1, a, 0));                  // no bytes
  CHECK(t.get(s1, &s) && s.ws == b && s.bytes == 32);   // ... and the entry is as it was
  CHECK(t.put(s0, nullptr, 0));             // forget
  CHECK(!t.get(s0, &s));
  CHECK(t.put(s0, nullptr, 0));             // forgetting an unknown stream is fine
  CHECK(t.size() == 1);

  // many streams, from several threads at once
  {
    DetTable m;
    std::vector<std::thread> th;
    for (int k = 0; k < 8; ++k)
      th.emplace_back([&m, k] {
        for (int i = 0; i < 200; ++i) {
          void* st = reinterpret_cast<void*>((unsigned long long)(0x100 * (k + 1) + 0x10 * (i % 5)));
          m.put(st, a, 16 + i);
          DetSlot q;
          if (m.get(st, &q) && q.ws != a) std::abort();
          if (i % 7 == 0) m.put(st, nullptr, 0);
        }
      });
    for (auto& x : th) x.join();
    CHECK(m.size() <= 40);
  }

  // launch geometry and sizes (hand-computed)
  CHECK(ln_bwd_rows_per_wave(37, 512) == 4 && ln_bwd_grid(37, 512) == 3);
  CHECK(ln_bwd_rows_per_wave(12805, 512) == 5 && ln_bwd_grid(12805, 512) == 641);
  CHECK(ln_bwd_rows_per_wave(12805, 1024) == 7 && ln_bwd_grid(12805, 1024) == 458);
  CHECK(det_workspace_bytes(1, 37, 512) == 3ll * 3 * 512 * 4);
  CHECK(det_workspace_bytes(1, 12805, 512) == 641ll * 3 * 512 * 4);
  CHECK(det_workspace_bytes(1, 12805, 1024) == 458ll * 3 * 1024 * 4);
  CHECK(det_workspace_bytes(1, 12805, 4096) == -1);
  CHECK(det_workspace_bytes(2, 1000, 512) == 16ll * 512 * 4);
  CHECK(det_workspace_bytes(2, 1 << 20, 512) == 1024ll * 512 * 4);
  CHECK(det_workspace_bytes(3, 50, 512) == 50ll * 512 * 4);
  CHECK(det_workspace_bytes(4, 3 * 40 * 40, 2 * 16 + 2 * 128) == 256ll * 288 * 4);     // 4800 pairs: 300 iterations' worth, 256 workgroups
  CHECK(det_workspace_bytes(4, 100, 288) == 7ll * 288 * 4);
  CHECK(det_workspace_bytes(9, 1, 1) == -1 && det_workspace_bytes(2, 0, 4) == -1);

  // the split rule: as many splits as asked for when their slabs fit, fewer when not, never an empty split, one when < 2 fit
  const long long slab = 256ll * 256;
  CHECK(det_fit_splits(8, 65, slab, 32ll << 20) == 8);        // ceil(65 / ceil(65 / 8)) = ceil(65 / 9) = 8
  CHECK(det_fit_splits(8, 65, slab, 3 * slab * 4) == 3);
  CHECK(det_fit_splits(8, 65, slab, 2 * slab * 4 - 1) == 1);
  CHECK(det_fit_splits(8, 65, slab, 0) == 1);
  CHECK(det_fit_splits(4, 6, slab, 32ll << 20) == 3);         // 4 splits of 2 K-tiles would leave the fourth empty
  CHECK(det_fit_splits(16, 6, slab, 32ll << 20) == 6);
  CHECK(det_fit_splits(1, 6, slab, 32ll << 20) == 1);
  for (int sk = 1; sk <= 40; ++sk)
    for (int kt = 1; kt <= 70; ++kt) {
      const int r = det_fit_splits(sk, kt, slab, 5 * slab * 4);
      const int per = (kt + r - 1) / r;
      CHECK(r >= 1 && r <= sk && r <= 5 && (r - 1) * per < kt);   // the last split is not empty
    }

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
