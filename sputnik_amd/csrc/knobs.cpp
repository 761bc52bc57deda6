// sputnik-amd: the tuning knobs (api_internal.h KnobId) and the 4-wave
// kernel selection that is one of them.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "api_internal.h"
#include "dsd4w.h"

namespace sputnik_amd {

// ---- tuning knobs ---------------------------------------------------------
// Unsupported switches for same-process A/B experiments and tests (documented
// as such in include/sputnik_amd.h and INTEGRATION.md §6). Each starts from
// its environment variable, else its default, on first use; the C-ABI's
// sputnik_tuning_set() changes it at run time (process-wide). Defaults are
// the shipped configuration; nothing in a correct caller needs them.
struct KnobDef {
  const char *name;
  const char *env;
  int def, lo, hi;
};
static const KnobDef kKnobs[kNumKnobs] = {
    {"pairs", "SPUTNIK_AMD_PAIRS", 1, 0, 1},
    {"pair_xcd2", "SPUTNIK_AMD_PAIR_XCD2", 3, 0, 3},
    {"split", "SPUTNIK_AMD_SPLIT", 1, 0, 1},
    {"split_min_bn", "SPUTNIK_AMD_SPLIT_MIN_BN", 128, 0, 1 << 20},
    {"dsd4w", "SPUTNIK_AMD_DSD4W", 1, 0, 7},
    {"grouped_sdd", "SPUTNIK_AMD_GROUPED_SDD", 1, 0, 1},
    {"grouped_min_per_cu", "SPUTNIK_AMD_GROUPED_MIN_PER_CU", 4, 0, 1 << 20},
    {"tall", "SPUTNIK_AMD_TALL", 1, 0, 2},
    {"tall_persistent", "SPUTNIK_AMD_TALL_PERSISTENT", 1, 0, 1},
    {"dds_xcd2", "SPUTNIK_AMD_DDS_XCD2", 3, 0, 3},
    {"sdd4w_max_ld", "SPUTNIK_AMD_SDD4W_MAX_LD", 16384, 0, 1 << 30},
    {"pair_fault", "SPUTNIK_AMD_PAIR_FAULT", 0, 0, 1},
    // (off by default: every chunk of a K-split group waits for all of its
    // peers, so it needs the whole grid resident at once -- PrepareSddKsplit)
    {"sdd_ksplit", "SPUTNIK_AMD_SDD_KSPLIT", 1, 1, 8},
    {"sdd_ksplit_min_k", "SPUTNIK_AMD_SDD_KSPLIT_MIN_K", 6144, 512, 1 << 30},
    {"sdd_order", "SPUTNIK_AMD_SDD_ORDER", 1, 0, 4},
    {"tall4w", "SPUTNIK_AMD_TALL4W", 1, 0, 1},
    {"tall_flush_w", "SPUTNIK_AMD_TALL_FLUSH_W", 4, 0, 64},
    {"tall_odd_share", "SPUTNIK_AMD_TALL_ODD_SHARE", 120, 50, 200},
    {"min_handoff", "SPUTNIK_AMD_MIN_HANDOFF", 2, 1, 64},
    {"xcd_rows", "SPUTNIK_AMD_XCD_ROWS", 1, 0, 1},
    {"sdd_krot", "SPUTNIK_AMD_SDD_KROT", 0, 0, 4},
    // (2: NT only -- SDD NT 16384^3 dense 7603 -> 6934 us, config 4 in
    // MegaBlocks' w1 layout 812 -> 805 us, other NT shapes a tie; NN / TT
    // ties or noise, profiles/r06/ab/sdd_spread_ab.jsonl)
    {"sdd_spread", "SPUTNIK_AMD_SDD_SPREAD", 2, 0, 2},
    // (SDD NT / TT: B transposed first when its K N 2 bytes reach this many
    // MiB -- the MALL's 256 MB -- and the product is dense enough; 0 off)
    {"sdd_bt_min_mib", "SPUTNIK_AMD_SDD_BT_MIN_MIB", 256, 0, 1 << 20},
    // (grouped 4-wave SDD with K >= this: the rows past the groups' full
    // rounds go to an 8-wave launch of a block per workgroup; 0 off)
    {"sdd_tail_min_k", "SPUTNIK_AMD_SDD_TAIL_MIN_K", 8192, 0, 1 << 30},
    // (SDD epilogue products, RunSddEpilogue: 0 auto, 1 the fused epilogue of
    // the 8-wave kernel, 2 plain SDD plus the elementwise kernel)
    {"sdd_act_route", "SPUTNIK_AMD_SDD_ACT_ROUTE", 0, 0, 2},
};
constexpr int kKnobUnset = -0x7fffffff - 1;
static std::atomic<int> g_knobs[kNumKnobs];
static std::once_flag g_knobs_once;

static void InitKnobs() {
  std::call_once(g_knobs_once, [] {
    for (int i = 0; i < kNumKnobs; ++i) {
      const char *e = std::getenv(kKnobs[i].env);
      // (an unset, unparsable or out-of-range value means the default)
      char *end = nullptr;
      const long v0 = e != nullptr && *e != 0 ? std::strtol(e, &end, 10) : 0;
      const bool ok = e != nullptr && *e != 0 && end != nullptr && *end == 0 &&
                      v0 >= kKnobs[i].lo && v0 <= kKnobs[i].hi;
      const int v = ok ? (int)v0 : kKnobs[i].def;
      g_knobs[i].store(v, std::memory_order_relaxed);
    }
  });
}

int Knob(KnobId k) {
  InitKnobs();
  return g_knobs[k].load(std::memory_order_relaxed);
}

static int KnobIndex(const char *name) {
  if (name == nullptr) return -1;
  for (int i = 0; i < kNumKnobs; ++i)
    if (std::strcmp(name, kKnobs[i].name) == 0) return i;
  return -1;
}

int TuningGet(const char *name) {
  const int i = KnobIndex(name);
  return i < 0 ? kKnobUnset : Knob(static_cast<KnobId>(i));
}

int TuningSet(const char *name, int value) {
  const int i = KnobIndex(name);
  if (i < 0 || value < kKnobs[i].lo || value > kKnobs[i].hi) return kKnobUnset;
  InitKnobs();
  return g_knobs[i].exchange(value, std::memory_order_relaxed);
}

void SetPairFault(int on) { (void)TuningSet("pair_fault", on != 0 ? 1 : 0); }

// DSD NN kernel selection: the 4-wave hand-scheduled kernel (dsd4w.hip) where
// it applies, else the 8-wave block_gemm_kernel. Knob "dsd4w" 0 (tests and
// A/B) keeps the 8-wave kernel.
static int Dsd4wMode() { return Knob(kKnobDsd4w); }
bool Dsd4wEnabled() { return Dsd4wMode() != 0; }
// 2..7: wherever the kernel can run, whatever the density (tests, A/B), with
// epilogue 0 .. 5 (dsd4w.h LaunchDsd4w); 1: the default epilogue.
bool Dsd4wForced() { return Dsd4wMode() >= 2; }
int Dsd4wEpi() {
  const int m = Dsd4wMode();
  return m >= 2 ? m - 2 : kDsd4wDefaultEpi;
}
int SelectDsdKernel(int four_wave) {
  if (four_wave < 0) return Dsd4wMode();
  return TuningSet("dsd4w", four_wave > 7 ? 7 : four_wave);
}

}  // namespace sputnik_amd
