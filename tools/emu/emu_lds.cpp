// tools/emu: storage behind the kernels' dynamic LDS arrays (`extern __shared__ T name[]`) in the host functional model
#include <stdint.h>
namespace ksk {
thread_local unsigned long long s_test[64 * 1024 / 8];
thread_local unsigned long long s_bt[64 * 1024 / 8];
thread_local uint32_t s_tot[64 * 1024 / 4];
}  // namespace ksk
namespace ksrs {
thread_local uint32_t s_hist[64 * 1024 / 4];
}  // namespace ksrs

// The runtime stand-in's ledger and its failure injection (hip/hip_runtime.h, README.md), for tests/test_ownership_emu.py.
// Exported by the functional model only: no part of include/ks_hip.h.
#include "hip/hip_runtime.h"
extern "C" {
// out: live hipMalloc + hipHostMalloc blocks | their bytes | live events | live streams | allocations made so far
void ks_emu_ledger(long long out[5]) {
  emu::Ledger& L = emu::g_ledger;
  std::lock_guard<std::mutex> lk(L.mu);
  out[0] = (long long)L.live.size();
  out[1] = L.bytes;
  out[2] = L.events.load();
  out[3] = L.streams.load();
  out[4] = L.allocations;
}
// the k-th allocation from now on (0 = the next one) returns hipErrorOutOfMemory, once; k < 0 disarms.  Returns 1 while a
// failure armed earlier has not fired yet.
int ks_emu_fail_alloc(long long k) {
  emu::Ledger& L = emu::g_ledger;
  std::lock_guard<std::mutex> lk(L.mu);
  const int pending = L.fail_in >= 0;
  L.fail_in = k < 0 ? -1 : k;
  return pending;
}
}
