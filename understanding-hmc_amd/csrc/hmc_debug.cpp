// hmc_debug.cpp — host side of the debug build's profiling hooks (hmc_debug.hpp): the environment
// variables and the stamp buffer.  Empty in the release library.
#include "hmc_debug.hpp"

#ifdef HMC_DEBUG_HOOKS
#include <cstdlib>

namespace hmc {

namespace {
unsigned long long* g_stamps = nullptr;   // HMC_DEBUG_STAMPS buffer of the last launch's arguments
int64_t g_stamp_waves = 0;

int env_int(const char* name, int unset) {
  const char* v = getenv(name);
  return v ? atoi(v) : unset;
}
}  // namespace

bool instrumented() { return env_int("HMC_DEBUG_ABLATE", 0) != 0 || env_int("HMC_DEBUG_L", -1) >= 0; }

void apply_env(RandArgs& a, const Layout& lay, int64_t n_chains) {
  a.dbg = env_int("HMC_DEBUG_ABLATE", 0);
  a.dbgL = env_int("HMC_DEBUG_L", -1);
  if (getenv("HMC_DEBUG_STAMPS")) {
    // one row per wave; the dense and NUTS argument blocks carry no lane-group layout and run 16
    // chain slots per wave
    const int cpw = lay.cpw > 0 ? lay.cpw : 16;
    const int64_t waves = (n_chains + cpw - 1) / cpw;
    if (g_stamps) (void)hipFree(g_stamps);
    g_stamps = nullptr;
    g_stamp_waves = waves;
    if (hipMalloc(&g_stamps, waves * kStampWords * sizeof(unsigned long long)) == hipSuccess) a.stamps = g_stamps;
  }
}

int force_K() { return env_int("HMC_FORCE_K", 0); }

bool force_group() {
  const char* kern = getenv("HMC_KERNEL");
  return kern && kern[0] == 'g';
}

}  // namespace hmc

// Copy the per-wave phase timers of the last HMC_DEBUG_STAMPS launch to the host; returns the words copied.
extern "C" int64_t hmc_debug_stamps(unsigned long long* host, int64_t cap_words) {
  using namespace hmc;
  if (!g_stamps) return 0;
  const int64_t words = g_stamp_waves * kStampWords < cap_words ? g_stamp_waves * kStampWords : cap_words;
  if (hipDeviceSynchronize() != hipSuccess) return 0;
  if (hipMemcpy(host, g_stamps, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return words;
}
#endif
