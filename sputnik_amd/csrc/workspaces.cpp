// sputnik-amd: every piece of device memory the dispatcher keeps or borrows:
// the pair-balancing workspaces and tile counters per (device, stream) and
// per graph capture, the transposed-B buffers, the caller's registered
// workspaces, and the accounting around them.
//
// Locks: g_bt_mu is taken before g_pairs_mu, never the reverse; g_ws_mu is
// held only around its table, never over a launch.
#include <atomic>
#include <cstdint>
#include <type_traits>

#include "dispatch_internal.h"
#include "layout.h"
#include "sputnik/sputnik.h"

namespace sputnik_amd {

constexpr int kMaxDevices = 64;

// ---- allocation / synchronisation accounting ------------------------------
// g_incall_events: every hipMalloc, hipFree, hipStreamSynchronize and
// hipDeviceSynchronize the library executes while a product entry point (a
// Run* function) is on this thread's stack; g_bt_launches: every
// LaunchTranspose16 enqueued for a product. Both only grow
// (sputnik_incall_events / sputnik_bt_launches): a caller, or a test, reads
// them around a call to see that the call allocated and synchronised nothing.
static std::atomic<unsigned long long> g_incall_events{0};
static std::atomic<unsigned long long> g_bt_launches{0};
static thread_local int t_product_depth = 0;
InProduct::InProduct() { ++t_product_depth; }
InProduct::~InProduct() { --t_product_depth; }
// Called right before each such HIP call.
static void InCallEvent() {
  if (t_product_depth > 0) g_incall_events.fetch_add(1, std::memory_order_relaxed);
}
unsigned long long InCallEvents() { return g_incall_events.load(std::memory_order_relaxed); }
unsigned long long BtLaunches() { return g_bt_launches.load(std::memory_order_relaxed); }

// Compute units of a device, queried once per device (every SDD and every
// pair-eligible DSD/DDS call needs it).
int DeviceCUs(int dev) {
  static int cached[kMaxDevices] = {};
  if (dev < 0 || dev >= kMaxDevices) return 0;
  int cus = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
  if (cus > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess || cus <= 0)
    return 0;
  __atomic_store_n(&cached[dev], cus, __ATOMIC_RELAXED);
  return cus;
}

// ---- pair-balancing workspace ---------------------------------------------
// fp32 partial slots + hand-off flags + an error word, one set per (device,
// stream) so concurrent streams never share them. Allocated on the first
// eligible call and kept for the life of the process (like a BLAS handle's
// workspace). One workspace per stream relies on stream order: launches on
// one stream never overlap, so each launch owns the slots while it runs.
// Every launch carries a new epoch; a consumer waits for its own epoch, so a
// flag left by an earlier launch (or by a producer that published after its
// consumer gave up) can never satisfy a later launch, and nothing has to be
// reset. A launch captured into a graph replays one set of arguments and
// may replay on any stream, so captured launches get a workspace of their
// own per (device, capture, capturing stream) and keep their epoch on the
// device (GemmParams::pair_sync): replays of one graph are ordered behind
// each other, and no eager launch or other capture shares that workspace.
// Key of every slot table: the (device, stream) a slot serves, and for the
// capture tables the capture it was made for.
struct SlotKey {
  int device = -1;
  hipStream_t stream = nullptr;
  unsigned long long capture = 0;  // capture id (capture tables only)
};
// Capture-table slots: set (by a user-object destructor on HIP's callback
// thread) once the captured graph and every executable made from it are
// destroyed; the slot is then re-tied to the next capture that needs one
// (WalkSlots) or freed by sputnik_capture_workspaces().
struct CaptureTied {
  std::atomic<int> released{0};
};
struct PairSlot : SlotKey, CaptureTied {
  float *partials = nullptr;
  unsigned *flags = nullptr;  // [pairs] flags, the error word, [epoch, count]
  unsigned epoch = 0;
  int pairs = 0;  // capacity
  int slots = 0;  // resident workgroups on the device
  bool used() const { return partials != nullptr; }
};
constexpr int kMaxPairSlots = 16;
constexpr int kMaxCaptureSlots = 64;
static PairSlot g_pairs[kMaxPairSlots];
static PairSlot g_capture_pairs[kMaxCaptureSlots];
// Guards the pair and counter tables; taken after g_bt_mu, never before it.
static std::mutex g_pairs_mu;

// Tile counter pair of persistent tall launches, per (device, stream): the
// kernel resets it to zero at the end of every launch (GemmParams::
// tile_counter), so launches on one stream need no host-side bookkeeping.
// Not used under graph capture (a replay on another stream could overlap an
// eager launch on this one) nor on hipStreamPerThread, whose one handle
// stands for many concurrently running streams.
struct CounterSlot : SlotKey, CaptureTied {
  unsigned long long *counter = nullptr;  // [fetch, done]
  bool used() const { return counter != nullptr; }
};
static CounterSlot g_counters[kMaxPairSlots];
static CounterSlot g_capture_counters[kMaxCaptureSlots];

// Capture status of `stream`: 0 not capturing, 1 capturing (id in *id),
// -1 the query failed or the capture is invalidated (no workspace then).
static int CaptureState(hipStream_t stream, unsigned long long *id) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  *id = 0;
  if (hipStreamGetCaptureInfo(stream, &cs, id) != hipSuccess) return -1;
  if (cs == hipStreamCaptureStatusNone) return 0;
  return cs == hipStreamCaptureStatusActive ? 1 : -1;
}

// Device memory for a workspace, zero-filled, callable while `stream` is
// being captured: the thread switches to relaxed capture mode (hipMalloc is
// not a stream operation), and the fill runs on a private non-blocking
// stream that no capture touches, synchronized before returning.
// The library's private non-blocking stream of a device (created on first
// use, kept for the process; caller holds g_pairs_mu).
static hipStream_t g_side[kMaxDevices] = {};
static hipError_t SideStream(int dev, hipStream_t *out) {
  if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
  if (g_side[dev] == nullptr) {
    const hipError_t e = hipStreamCreateWithFlags(&g_side[dev], hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  *out = g_side[dev];
  return hipSuccess;
}

static hipError_t AllocZeroed(void **ptr, size_t bytes, int dev) {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  hipStream_t side = nullptr;
  hipError_t e = SideStream(dev, &side);
  *ptr = nullptr;
  if (e == hipSuccess) {
    InCallEvent();
    e = hipMalloc(ptr, bytes);
  }
  if (e == hipSuccess) e = hipMemsetAsync(*ptr, 0, bytes, side);
  if (e == hipSuccess) {
    InCallEvent();
    e = hipStreamSynchronize(side);
  }
  if (e != hipSuccess && *ptr != nullptr) {
    InCallEvent();
    (void)hipFree(*ptr);
    *ptr = nullptr;
  }
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  return e;
}

// Ties a capture-table slot to the lifetime of the graph being captured on
// `stream`: a user object retained by the graph (executables instantiated
// from it retain it too) sets *released when the last reference goes, i.e.
// once the graph and all its executables are destroyed and no launch of them
// is pending. A destructor may not call HIP, so the memory is freed later by
// ReclaimCaptureSlots. Returns false if the graph cannot be tied (the slot
// then lives for the process, as before).
static void MarkReleased(void *flag) {
  static_cast<std::atomic<int> *>(flag)->store(1, std::memory_order_release);
}
static bool TieToCapturedGraph(hipStream_t stream, std::atomic<int> *released) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t *deps = nullptr;
  size_t ndeps = 0;
  if (hipStreamGetCaptureInfo_v2(stream, &cs, &id, &graph, &deps, &ndeps) !=
          hipSuccess ||
      cs != hipStreamCaptureStatusActive || graph == nullptr)
    return false;
  hipUserObject_t obj = nullptr;
  if (hipUserObjectCreate(&obj, released, MarkReleased, 1,
                          hipUserObjectNoDestructorSync) != hipSuccess)
    return false;
  // Move our one reference into the graph: the graph now owns the object.
  if (hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove) !=
      hipSuccess) {
    (void)hipUserObjectRelease(obj, 1);
    return false;
  }
  return true;
}

// Frees the capture-table workspaces whose graphs are gone (caller holds
// g_pairs_mu; called from eager launches only, never while this thread's
// stream is being captured, since hipFree is not a capturable call).
static void FreeQuiet(void *ptr) {
  if (ptr == nullptr) return;
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  (void)hipThreadExchangeStreamCaptureMode(&mode);
  InCallEvent();
  (void)hipFree(ptr);
  (void)hipThreadExchangeStreamCaptureMode(&mode);
}

// A (device, stream) table ran out of slots: the caller falls back to the
// plain launch (correct, slower); said once per process.
// kind: 0 pair balancing, 1 persistent launches; +2 in captured graphs.
static void WarnSlotsFull(int kind) {
  static bool warned[4] = {false, false, false, false};
  static const char *const what[4] = {
      "streams use pair balancing", "streams use persistent launches",
      "graph captures use pair balancing",
      "graph captures use persistent launches"};
  if (kind >= 0 && kind < 4 && !warned[kind]) {
    warned[kind] = true;
    SPUTNIK_LOG(WARNING) << "sputnik-amd: more than "
                         << (kind < 2 ? kMaxPairSlots : kMaxCaptureSlots)
                         << " " << what[kind]
                         << "; further ones run without it";
  }
}

// The one walk over a slot table (the caller holds the table's lock): the
// slot in use for `key`; else, for a capture, a slot of the device whose
// graph is gone (re-tied to the capture under way unless `dry`; its memory
// stays as it is, no HIP free on this path: frees happen in
// sputnik_capture_workspaces()); else, with `claim`, the first free slot,
// *fresh set: the caller fills it (or, dry, describes what it would hold).
// nullptr: none.
template <class Slot>
static Slot *WalkSlots(Slot *table, int n, const SlotKey &key, bool capturing, bool dry,
                       bool claim, bool *fresh) {
  *fresh = false;
  for (int i = 0; i < n; ++i) {
    Slot &s = table[i];
    if (s.used() && s.device == key.device && s.stream == key.stream &&
        s.capture == key.capture)
      return &s;
  }
  if constexpr (std::is_base_of<CaptureTied, Slot>::value) {
    if (capturing) {
      for (int i = 0; i < n; ++i) {
        Slot &s = table[i];
        if (s.used() && s.device == key.device &&
            s.released.load(std::memory_order_acquire) != 0) {
          if (dry) return &s;
          static_cast<SlotKey &>(s) = key;
          s.released.store(0, std::memory_order_relaxed);
          (void)TieToCapturedGraph(key.stream, &s.released);
          return &s;
        }
      }
    }
  }
  if (!claim) return nullptr;
  for (int i = 0; i < n; ++i)
    if (!table[i].used()) {
      *fresh = true;
      return &table[i];
    }
  return nullptr;
}

// A re-tied capture-table pair slot keeps its memory and device epoch word:
// the word only ever grows, so the flags the old graph left can never match a
// new launch, and its arrival count is back at zero (the last arriver of
// every launch resets it).
// (caller holds g_pairs_mu; dry: a slot that would be allocated is described
// in *dry_slot)
static PairSlot *AcquirePairSlot(hipStream_t stream, bool dry, PairSlot *dry_slot,
                                 int *capturing_out) {
  SlotKey key;
  key.stream = stream;
  const int capturing = CaptureState(stream, &key.capture);
  *capturing_out = capturing;
  if (capturing < 0) return nullptr;
  if (hipGetDevice(&key.device) != hipSuccess) return nullptr;
  bool fresh = false;
  PairSlot *slot = WalkSlots(capturing ? g_capture_pairs : g_pairs,
                             capturing ? kMaxCaptureSlots : kMaxPairSlots, key,
                             capturing != 0, dry, /*claim=*/true, &fresh);
  if (slot == nullptr) {
    if (!dry) WarnSlotsFull(capturing ? 2 : 0);
    return nullptr;
  }
  if (!fresh) return slot;
  const int dev = key.device, cus = DeviceCUs(dev);
  if (cus <= 0) return nullptr;
  const int slots = cus * CfgSparse::kWGs;
  // Partial slots of 128 x 512 fp32 (256 KiB): one per resident workgroup
  // (a pair uses one per pair, split mode one per tile, the SDD K-split one
  // per workgroup): 64 MiB per workspace on MI355X. Flags: [pairs] pair
  // flags, the error word, [epoch, count] (pair_sync), [slots] K-split flags.
  const int pairs = slots / 2;
  if (dry) {  // the workspace a launch would allocate
    dry_slot->slots = slots;
    dry_slot->pairs = pairs;
    return dry_slot;
  }
  void *partials = nullptr, *flags = nullptr;
  if (AllocZeroed(&partials, (size_t)slots * kBM * CfgSparse::kBN * sizeof(float), dev) !=
      hipSuccess)
    return nullptr;
  if (AllocZeroed(&flags, (pairs + 3 + slots) * sizeof(unsigned), dev) != hipSuccess) {
    FreeQuiet(partials);
    return nullptr;
  }
  static_cast<SlotKey &>(*slot) = key;
  slot->partials = static_cast<float *>(partials);
  slot->flags = static_cast<unsigned *>(flags);
  slot->pairs = pairs;
  slot->slots = slots;
  slot->released.store(0, std::memory_order_relaxed);
  if (capturing) (void)TieToCapturedGraph(stream, &slot->released);
  return slot;
}

int BindPairWorkspace(GemmParams *p, long long need, hipStream_t stream, bool dry) {
  std::lock_guard<std::mutex> lock(g_pairs_mu);
  PairSlot dry_slot;
  int capturing = 0;
  PairSlot *slot = AcquirePairSlot(stream, dry, &dry_slot, &capturing);
  if (slot == nullptr || need > slot->slots) return 0;
  if (dry) return slot->slots;
  if (++slot->epoch == 0) slot->epoch = 1;  // 0 is the initial flag value
  p->pair_partials = slot->partials;
  p->pair_flags = slot->flags;
  p->pair_epoch = slot->epoch;
  p->pair_error = slot->flags + slot->pairs;
  p->pair_sync = capturing ? slot->flags + slot->pairs + 1 : nullptr;
  p->ks_flags = slot->flags + slot->pairs + 3;
  return slot->slots;
}

// Pair hand-offs that timed out (and were recomputed by their consumer)
// since the last call, summed over every workspace of the current device;
// the error words are cleared. One device-wide
// synchronize first: the streams the workspaces were made for may have been
// destroyed since (or their handles reused), so they are never used here.
int PairErrors() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  std::lock_guard<std::mutex> lock(g_pairs_mu);
  int total = 0;
  for (int i = 0; i < kMaxPairSlots + kMaxCaptureSlots; ++i) {
    PairSlot &s = i < kMaxPairSlots ? g_pairs[i]
                                    : g_capture_pairs[i - kMaxPairSlots];
    if (s.partials == nullptr || s.device != dev) continue;
    unsigned word = 0;
    if (hipMemcpy(&word, s.flags + s.pairs, sizeof(word),
                  hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    if (word != 0) {
      total += (int)word;
      const unsigned zero = 0;
      if (hipMemcpy(s.flags + s.pairs, &zero, sizeof(zero),
                    hipMemcpyHostToDevice) != hipSuccess)
        return -1;
    }
  }
  return total;
}

static void ReclaimCaptureSlots() {
  for (auto &sl : g_capture_pairs) {
    if (sl.partials == nullptr ||
        sl.released.load(std::memory_order_acquire) == 0)
      continue;
    FreeQuiet(sl.partials);
    FreeQuiet(sl.flags);
    sl.partials = nullptr;
    sl.flags = nullptr;
    static_cast<SlotKey &>(sl) = SlotKey{};
    sl.epoch = 0;
    sl.pairs = sl.slots = 0;
    sl.released.store(0, std::memory_order_relaxed);
  }
  for (auto &c : g_capture_counters) {
    if (c.counter == nullptr || c.released.load(std::memory_order_acquire) == 0)
      continue;
    FreeQuiet(c.counter);
    c.counter = nullptr;
    static_cast<SlotKey &>(c) = SlotKey{};
    c.released.store(0, std::memory_order_relaxed);
  }
}

int CaptureWorkspaces() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lock(g_pairs_mu);
  ReclaimCaptureSlots();
  int n = 0;
  for (const auto &s : g_capture_pairs)
    n += s.partials != nullptr && s.device == dev;
  for (const auto &c : g_capture_counters)
    n += c.counter != nullptr && c.device == dev;
  return n;
}

void BindTileCounter(GemmParams *p, hipStream_t stream, bool dry) {
  // Persistent: one workgroup per slot; the first `slots` tiles go by
  // workgroup index, the rest are fetched from a per-stream counter. Short
  // tiles (most rows of a tall 2% operand hold 0-2 blocks) otherwise leave
  // ~20% of the slots idle between a workgroup's end and the next dispatch
  // (r02 timeline: 400-460 of 512 resident); a static tile stride instead
  // loses more to imbalance (403 vs 337 us, config 5).
  const int persistent = Knob(kKnobTallPersistent);
  SlotKey key;
  key.stream = stream;
  const int cus = hipGetDevice(&key.device) == hipSuccess ? DeviceCUs(key.device) : 0;
  const int slots = cus * CfgTall::kWGs;
  if (!persistent || slots <= 0 || p->num_tiles <= slots) return;
  if (stream == hipStreamPerThread) return;  // many streams, one handle
  // A captured launch gets a counter pair of its own capture (the kernel
  // leaves it at zero, so every replay starts clean; a released capture
  // slot is re-tied for the same reason).
  const int capturing = CaptureState(stream, &key.capture);
  if (capturing < 0) return;
  std::lock_guard<std::mutex> lock(g_pairs_mu);
  bool fresh = false;
  CounterSlot *slot = WalkSlots(capturing ? g_capture_counters : g_counters,
                                capturing ? kMaxCaptureSlots : kMaxPairSlots, key,
                                capturing != 0, dry, /*claim=*/true, &fresh);
  if (slot == nullptr) {
    if (!dry) WarnSlotsFull(capturing ? 3 : 1);
    return;
  }
  if (fresh) {
    if (dry) {  // the counter a launch would allocate
      p->grid = slots;
      p->persistent = 1;
      return;
    }
    void *ctr = nullptr;
    if (AllocZeroed(&ctr, 2 * sizeof(unsigned long long), key.device) != hipSuccess)
      return;
    static_cast<SlotKey &>(*slot) = key;
    slot->counter = static_cast<unsigned long long *>(ctr);
    slot->released.store(0, std::memory_order_relaxed);
    if (capturing) (void)TieToCapturedGraph(stream, &slot->released);
  }
  p->grid = slots;
  p->persistent = 1;
  p->tile_counter = slot->counter;
}

// ---- SDD with B stored transposed, over operands past the MALL -------------
// SDD NT / TT read B^T's rows 256 B per k-block. While A and B fit the
// 256-MB Infinity Cache (MALL) that costs nothing (NT 8192^3 runs at NN's
// speed), past it the misses go to HBM: SDD NT 16384^3 at 50% ran 5231 us
// against NN's 3516. There, B is transposed
// once into a library-owned buffer ([K][N], layout.hip, ~2 K N 2 bytes of
// HBM traffic) and the N-major kernel (NN / TN) runs on it (the gates are
// dispatch.cpp's BtAppliesSdd / BtAppliesDsd over BtGate below). On the
// library route, eager launches only: a stream being captured keeps the NT /
// TT kernel (the buffer is allocated on first use). One buffer per (device,
// stream), grown as needed, kept until sputnik_release_workspaces()
// (INTEGRATION.md 3b); stream order makes it safe to reuse. A caller who
// supplies the memory (below) gets the same two launches with none of this.
struct BtSlot : SlotKey {
  void *data = nullptr;
  size_t bytes = 0;
  bool used() const { return data != nullptr; }
};
static BtSlot g_bt[kMaxPairSlots];
// Held from choosing the buffer until the transpose and the product are
// enqueued, so another thread cannot grow (free) the buffer of the same
// stream in between; taken before g_pairs_mu, never while holding it.
static std::mutex g_bt_mu;

bool BtGate(const Matrix &b) {
  const long long min_mib = Knob(kKnobSddBtMinMib);
  if (min_mib <= 0) return false;
  const long long n = b.rows, k = b.cols;  // B^T stored [N][K]
  // (layout.hip moves 16-byte vectors: a 16-byte aligned B)
  return n % 64 == 0 && k % 64 == 0 && n * k * 2 >= (min_mib << 20) &&
         (reinterpret_cast<uintptr_t>(b.data) & 15) == 0;
}

bool BtLibraryStreamOk(hipStream_t stream) {
  if (stream == hipStreamPerThread) return false;
  unsigned long long id = 0;
  return CaptureState(stream, &id) == 0;
}

size_t BtBytes(const Matrix &b) {
  return (((size_t)b.rows * b.cols * 2) + 255) & ~(size_t)255;
}

// ---- caller-owned transposed-B workspaces ----------------------------------
// The reference hands every workspace to the caller (arguments.h); here the
// caller may hand over the memory of the transposed copy, per call (the *_ws
// entry points) or per (device, stream) (sputnik_set_stream_workspace, for
// callers bound to the reference's Matmul / MatmulEx signatures). With such
// memory a product takes no g_bt_mu, touches no BtSlot, allocates, frees and
// synchronises nothing, and runs the same two launches while `stream` is
// being captured or is hipStreamPerThread. A stream with a registration
// never uses the library-owned buffer: memory that is too small or not
// 16-byte aligned keeps the NT / TT kernel.
struct WsReg : SlotKey {
  void *ptr = nullptr;  // nullptr: free entry
  size_t bytes = 0;
  bool used() const { return ptr != nullptr; }
};
static WsReg g_ws[kMaxPairSlots];
static std::mutex g_ws_mu;  // held only around the table, never over a launch

hipError_t SetStreamWorkspace(hipStream_t stream, void *ptr, size_t bytes) {
  // (hipStreamPerThread names a different stream in every thread: there is
  // no one stream whose order would protect the memory)
  if (stream == hipStreamPerThread) return hipErrorInvalidValue;
  if (ptr != nullptr && (bytes == 0 || (reinterpret_cast<uintptr_t>(ptr) & 15) != 0))
    return hipErrorInvalidValue;
  SlotKey key;
  key.stream = stream;
  const hipError_t e = hipGetDevice(&key.device);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_ws_mu);
  bool fresh = false;
  WsReg *slot = WalkSlots(g_ws, kMaxPairSlots, key, false, false, /*claim=*/ptr != nullptr,
                          &fresh);
  if (ptr == nullptr) {
    if (slot != nullptr) *slot = WsReg{};
    return hipSuccess;
  }
  if (slot == nullptr) return hipErrorOutOfMemory;
  static_cast<SlotKey &>(*slot) = key;
  slot->ptr = ptr;
  slot->bytes = bytes;
  return hipSuccess;
}

// The workspace of this call: the caller's own, else the one registered for
// (current device, stream). false: neither (the library route).
static bool CallerWorkspace(hipStream_t stream, Workspace given, Workspace *out) {
  if (given.ptr != nullptr && given.bytes != 0) {
    *out = given;
    return true;
  }
  if (stream == hipStreamPerThread) return false;
  SlotKey key;
  key.stream = stream;
  if (hipGetDevice(&key.device) != hipSuccess) return false;
  std::lock_guard<std::mutex> lock(g_ws_mu);
  bool fresh = false;
  const WsReg *r = WalkSlots(g_ws, kMaxPairSlots, key, false, false, /*claim=*/false, &fresh);
  if (r == nullptr) return false;
  out->ptr = r->ptr;
  out->bytes = r->bytes;
  return true;
}

static bool WorkspaceFits(Workspace ws, size_t bytes) {
  return ws.bytes >= bytes && (reinterpret_cast<uintptr_t>(ws.ptr) & 15) == 0;
}

// B^T ([rows][cols]) transposed into `out` on `stream`, counted.
static hipError_t EnqueueBt(const Matrix &b, void *out, hipStream_t stream) {
  g_bt_launches.fetch_add(1, std::memory_order_relaxed);
  return LaunchTranspose16(b.data, b.rows, b.cols, out, stream);
}

// The transposed-B buffer of (device, stream), at least `bytes` (nullptr:
// none -- the table is full or the allocation failed; the caller keeps the
// NT / TT kernel). Caller holds g_bt_mu.
static void *BtBuffer(hipStream_t stream, size_t bytes) {
  SlotKey key;
  key.stream = stream;
  if (hipGetDevice(&key.device) != hipSuccess) return nullptr;
  bool fresh = false;
  BtSlot *slot = WalkSlots(g_bt, kMaxPairSlots, key, false, false, /*claim=*/true, &fresh);
  if (slot == nullptr) return nullptr;
  if (slot->bytes < bytes) {
    if (slot->data != nullptr) {
      // the stream's earlier launches may still read the old buffer
      InCallEvent();
      if (hipStreamSynchronize(stream) != hipSuccess) return nullptr;
      FreeQuiet(slot->data);
      slot->data = nullptr;
      slot->bytes = 0;
    }
    InCallEvent();
    if (hipMalloc(&slot->data, bytes) != hipSuccess) {
      slot->data = nullptr;
      return nullptr;
    }
    slot->bytes = bytes;
    static_cast<SlotKey &>(*slot) = key;
  }
  return slot->data;
}

BtCopy TransposeB(const Matrix &b, hipStream_t stream, Workspace ws) {
  BtCopy copy;
  const size_t bt_bytes = (size_t)b.rows * b.cols * 2;
  Workspace own;
  if (CallerWorkspace(stream, ws, &own)) {
    // the caller's memory: no lock, no slot, captured or not; memory that
    // does not fit keeps the NT / TT kernel
    if (WorkspaceFits(own, bt_bytes)) copy.data = own.ptr;
  } else if (BtLibraryStreamOk(stream)) {
    copy.lock = std::unique_lock<std::mutex>(g_bt_mu);
    copy.data = BtBuffer(stream, bt_bytes);
    if (copy.data == nullptr) copy.lock.unlock();
  }
  if (copy.data != nullptr) copy.error = EnqueueBt(b, copy.data, stream);
  return copy;
}

// Device memory the library holds on the current device: transposed-B
// buffers, eager and capture pair workspaces, tile counters (host only).
size_t RetainedBytes() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  size_t total = 0;
  {
    std::lock_guard<std::mutex> lock(g_bt_mu);
    for (const BtSlot &s : g_bt)
      if (s.data != nullptr && s.device == dev) total += s.bytes;
  }
  std::lock_guard<std::mutex> lock(g_pairs_mu);
  for (int i = 0; i < kMaxPairSlots + kMaxCaptureSlots; ++i) {
    const PairSlot &s = i < kMaxPairSlots ? g_pairs[i] : g_capture_pairs[i - kMaxPairSlots];
    if (s.partials == nullptr || s.device != dev) continue;
    // (the sizes AcquirePairSlot allocates)
    total += (size_t)s.slots * kBM * CfgSparse::kBN * sizeof(float) +
             (size_t)(s.pairs + 3 + s.slots) * sizeof(unsigned);
  }
  for (int i = 0; i < kMaxPairSlots + kMaxCaptureSlots; ++i) {
    const CounterSlot &c =
        i < kMaxPairSlots ? g_counters[i] : g_capture_counters[i - kMaxPairSlots];
    if (c.counter != nullptr && c.device == dev) total += 2 * sizeof(unsigned long long);
  }
  return total;
}

// Frees every library-owned transposed-B buffer of the current device after
// one device-wide synchronize (the streams the buffers were made for may be
// gone, as in PairErrors) and returns the bytes freed; the next library-route
// launch allocates again. The lock is held across the synchronize, so no
// library-route product can enqueue work on a buffer between the two. Pair
// workspaces and tile counters stay: their epochs live in them.
size_t ReleaseWorkspaces() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(g_bt_mu);
  if (hipDeviceSynchronize() != hipSuccess) return 0;
  size_t freed = 0;
  for (BtSlot &s : g_bt) {
    if (s.data == nullptr || s.device != dev) continue;
    FreeQuiet(s.data);
    freed += s.bytes;
    s = BtSlot{};
  }
  return freed;
}

}  // namespace sputnik_amd
