// device_mem_check.cpp — csrc/device_mem.h, and the solver handle built from it (csrc/hdsm_handle.h), on the host
// (HDSM_DEVICE_MEM_HOST: blocks, events and streams are malloc'ed and counted, the k-th allocation can be made to fail).
// Stand-alone; built with the address and undefined-behaviour sanitizers by tests/test_device_mem.py.
// Every property is an assertion of this program (CHECK): nothing is left to a leak report. Exit status 0 = all held.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <new>

#include "../multi_agent_pkgs_amd/csrc/device_mem.h"
#include "../multi_agent_pkgs_amd/csrc/hdsm_handle.h"

// The seam does not cover recording and reading events, and nothing of the HIP runtime is linked: the three calls TimedInterval
// makes are defined here and count themselves.
static int g_event_calls = 0;
extern "C" hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return ++g_event_calls, hipSuccess; }
extern "C" hipError_t hipEventSynchronize(hipEvent_t) { return ++g_event_calls, hipSuccess; }
extern "C" hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { return *ms = 0.25f, ++g_event_calls, hipSuccess; }

using hdsm_mem::DevBuf;
using hdsm_mem::g_fail_in;
using hdsm_mem::g_live;
using hdsm_mem::g_syncs;
using hdsm_handle::Handle;

static int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++g_failed; \
  } while (0)

// six buffers in groups, shaped like DSwarm: the core ones, a nested opt-in group, an array of events that nobody creates
struct Group {
  DevBuf<double> d_a;
  DevBuf<int32_t> d_b;
};
struct Owner {
  DevBuf<double> d_x;
  DevBuf<int32_t> d_y;
  DevBuf<uint8_t> d_z, d_w;
  Group g;
  hdsm_mem::DevEvent ev[8];
  hdsm_mem::TimedInterval timed;
};

// hdsm_dswarm_create's shape: the object in a unique_ptr, every failure "return the code"
static hipError_t create(Owner** out) {
  *out = nullptr;
  std::unique_ptr<Owner> o(new (std::nothrow) Owner);
  if (!o) return hipErrorOutOfMemory;
  hdsm_mem::FirstError ok;
  ok(o->d_x.alloc_zeroed(5)), ok(o->d_y.alloc_zeroed(0)), ok(o->d_z.alloc_zeroed(3)), ok(o->d_w.alloc(7));
  if (!ok.ok()) return ok.e;
  if (hipError_t e = o->g.d_a.alloc_zeroed(2)) return e;
  if (hipError_t e = o->g.d_b.alloc(4)) return e;
  *out = o.release();
  return hipSuccess;
}

// the solver handle with small sizes, as hdsm_create leaves it in front of alloc_fixed()
static std::unique_ptr<Handle> small_handle() {
  std::unique_ptr<Handle> h(new Handle);
  h->max_inst = 3, h->n_rob_max = 5, h->N = 10, h->P = 4, h->RS = 18, h->n = 30;
  h->cus = 2, h->rec_cap = 8, h->scratch_stride = 16;
  return h;
}
static const hdsm::Shape ITEMS = hdsm::SHAPE_duo;  // (pass 2 of a split launch at n <= 30)

// the raw allocations `f` makes when none fails (counted with the knob itself: armed far beyond them)
template <class F>
static long count_allocs(F f) {
  g_fail_in = 1 << 20;
  CHECK(f() == hipSuccess);
  const long k = (1 << 20) - g_fail_in;
  g_fail_in = 0;
  return k;
}

static void check_new_owners() {
  {  // GrowBuf: grows by reallocating behind one synchronisation of the stream, never shrinks, forgets its capacity with its block
    hdsm_mem::GrowBuf<double> g;
    const long s0 = g_syncs;
    CHECK(g.get() == nullptr && g.capacity() == 0 && g.ensure(0, nullptr) == hipSuccess && g.get() == nullptr && g_live == 0 && g_syncs == s0);
    CHECK(g.ensure(8, nullptr) == hipSuccess && g.capacity() == 8 && g_live == 1 && g_syncs == s0 + 1);
    double* p = g.get();
    p[7] = 1.0;
    CHECK(g.ensure(8, nullptr) == hipSuccess && g.ensure(3, nullptr) == hipSuccess && g.get() == p && g.capacity() == 8 && g_live == 1 && g_syncs == s0 + 1);
    CHECK(g.ensure(100, nullptr) == hipSuccess && g.capacity() == 100 && g_live == 1 && g_syncs == s0 + 2);
    g.get()[99] = 1.0;
    g_fail_in = 1;
    CHECK(g.ensure(200, nullptr) == hipErrorOutOfMemory && g.get() == nullptr && g.capacity() == 0 && g_live == 0);
    CHECK(g.ensure(4, nullptr) == hipSuccess && g.get() != nullptr && g.capacity() == 4 && g_live == 1);  // (allocates again)
    p = g.get();
    hdsm_mem::GrowBuf<double> m(std::move(g));
    CHECK(m.get() == p && m.capacity() == 4 && g.get() == nullptr && g.capacity() == 0 && g_live == 1);
    hdsm_mem::GrowBuf<double> k;
    CHECK(k.ensure(2, nullptr) == hipSuccess && g_live == 2);
    k = std::move(m);
    CHECK(k.get() == p && k.capacity() == 4 && m.get() == nullptr && m.capacity() == 0 && g_live == 1);
    CHECK(m.ensure(1, nullptr) == hipSuccess && g_live == 2);  // (a moved-from one starts over)
  }
  CHECK(g_live == 0);
  {  // PinnedBuf: the same rules without a stream
    hdsm_mem::PinnedBuf b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.ensure(16) == hipSuccess && b.capacity() == 16 && g_live == 1);
    void* p = b.get();
    static_cast<char*>(p)[15] = 1;
    CHECK(b.ensure(8) == hipSuccess && b.get() == p && b.capacity() == 16 && g_live == 1);
    CHECK(b.ensure(64) == hipSuccess && b.capacity() == 64 && g_live == 1);
    static_cast<char*>(b.get())[63] = 1;
    g_fail_in = 1;
    CHECK(b.ensure(65) == hipErrorOutOfMemory && b.get() == nullptr && b.capacity() == 0 && g_live == 0);
    CHECK(b.ensure(8) == hipSuccess && b.capacity() == 8 && g_live == 1);
    p = b.get();
    hdsm_mem::PinnedBuf m(std::move(b));
    CHECK(m.get() == p && m.capacity() == 8 && b.get() == nullptr && b.capacity() == 0 && g_live == 1);
    CHECK(b.ensure(4) == hipSuccess && g_live == 2);
    b = std::move(m);
    CHECK(b.get() == p && b.capacity() == 8 && m.get() == nullptr && g_live == 1);
  }
  CHECK(g_live == 0);
  {  // MappedWord: zero at first, one word seen from both sides
    hdsm_mem::MappedWord w;
    CHECK(w.host() == nullptr && w.dev() == nullptr);
    CHECK(w.create() == hipSuccess && w.host() != nullptr && *w.host() == 0 && w.dev() == w.host() && g_live == 1);
    *w.dev() = 5;
    int32_t* p = w.host();
    hdsm_mem::MappedWord m(std::move(w));
    CHECK(m.host() == p && m.dev() == p && *m.host() == 5 && w.host() == nullptr && w.dev() == nullptr && g_live == 1);
    CHECK(w.create() == hipSuccess && g_live == 2);
    w = std::move(m);
    CHECK(w.host() == p && m.host() == nullptr && m.dev() == nullptr && g_live == 1);
    g_fail_in = 1;
    CHECK(m.create() == hipErrorOutOfMemory && m.host() == nullptr && m.dev() == nullptr && g_live == 1);
  }
  CHECK(g_live == 0);
  {  // DevStream, and the event with flags: created once, moved, empty after a failure
    hdsm_mem::DevStream a;
    CHECK(a.get() == nullptr && a.create() == hipSuccess && a.get() != nullptr && g_live == 1);
    hipStream_t s = a.get();
    CHECK(a.create() == hipSuccess && a.get() == s && g_live == 1);
    hdsm_mem::DevStream b(std::move(a));
    CHECK(b.get() == s && a.get() == nullptr && g_live == 1);
    CHECK(a.create() == hipSuccess && g_live == 2);
    a = std::move(b);
    CHECK(a.get() == s && b.get() == nullptr && g_live == 1);
    g_fail_in = 1;
    CHECK(b.create() == hipErrorOutOfMemory && b.get() == nullptr && g_live == 1);
    hdsm_mem::DevEvent e, f;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && e && g_live == 2);
    hipEvent_t ev = e.get();
    hdsm_mem::DevEvent m(std::move(e));
    CHECK(m.get() == ev && !e && g_live == 2);
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && g_live == 3);
    e = std::move(m);
    CHECK(e.get() == ev && !m && g_live == 2);
    g_fail_in = 1;
    CHECK(f.create(hipEventDisableTiming) == hipErrorOutOfMemory && !f && g_live == 2);
  }
  CHECK(g_live == 0);
}

static void check_handle() {
  long fixed = 0, split = 0;
  {  // nothing fails: what the kernels rely on is zero, the three words are there
    std::unique_ptr<Handle> h = small_handle();
    fixed = count_allocs([&] { return h->alloc_fixed(); });
    CHECK(fixed > 0 && g_live == fixed);
    bool zero = true;
    for (int i = 0; i < 8 * 3; ++i) zero = zero && h->d_stats.get()[i] == 0;
    for (int i = 0; i < (hdsm::MAXNV + 2) * 3; ++i) zero = zero && h->d_warm.get()[i] == 0;
    for (int i = 0; i < 5; ++i) zero = zero && h->d_zero.get()[i] == 0;
    for (int i = 0; i < 3 * 4 * 18; ++i) zero = zero && h->stage.d_b.get()[i] == 0.0 && h->stage.d_A.get()[3 * i + 2] == 0.0;
    for (int i = 0; i < 5 * 11 * 9; ++i) zero = zero && h->stage.d_plans.get()[i] == 0.0;
    CHECK(zero);
    h->d_scratch.get()[3 * 16 - 1] = 1.0, h->stage.d_traj.get()[3 * 11 * 9 - 1] = 1.0, h->pre.d_setup.get()[3 * hdsm::KROWS - 1] = 1.0;  // (whole blocks)
    CHECK(*h->ovf_flag.host() == 0 && *h->tree_flag.host() == 0 && *h->item_total.host() == 0 && h->ovf_flag.dev() != nullptr);
    CHECK(h->stream.get() != nullptr && h->ev_done && h->kernel_time.start && h->kernel_time.stop && !h->d_prof && !h->sub.ready());
  }
  CHECK(g_live == 0);
  for (long k = 1; k <= fixed; ++k) {  // hdsm_create with its k-th allocation failing: the error comes back, the unique_ptr releases the rest
    {
      std::unique_ptr<Handle> h = small_handle();
      g_fail_in = k;
      CHECK(h->alloc_fixed() != hipSuccess && g_fail_in == 0);
    }
    CHECK(g_live == 0);
  }
  {
    std::unique_ptr<Handle> h = small_handle();
    CHECK(h->alloc_fixed() == hipSuccess);
    split = count_allocs([&] { return h->sub.alloc(*h, ITEMS); });
    CHECK(split > 0 && g_live == fixed + split && h->sub.ready());
  }
  for (long k = 1; k <= split; ++k) {  // the first split launch with its k-th allocation failing: the handle goes on as it was
    std::unique_ptr<Handle> h = small_handle();
    CHECK(h->alloc_fixed() == hipSuccess);
    int32_t* const stats = h->d_stats.get();
    g_fail_in = k;
    CHECK(h->sub.alloc(*h, ITEMS) != hipSuccess && g_fail_in == 0);
    const hdsm_handle::SplitState& s = h->sub;
    CHECK(!s.ready() && s.rows_cap == 0 && s.items_cap == 0 && s.sub_slots_n == 0 && s.pool_cap == 0);
    CHECK(!s.d_recs && !s.d_rec_cand && !s.d_rec_mw && !s.d_rec_src && !s.d_rec_count && !s.d_items && !s.d_slot_busy && !s.d_split && !s.d_sub_stats);
    CHECK(!s.d_sub_warm && !s.d_sub_status && !s.d_inc && !s.d_node_pool && !s.d_sub_traj && !s.d_sub_ctrl && !s.d_sub_obj && !s.d_sub_scratch && !s.d_sub_used);
    CHECK(g_live == fixed && h->d_stats.get() == stats && stats[8 * 3 - 1] == 0 && h->stream.get() != nullptr && *h->tree_flag.host() == 0);
    CHECK(h->sub.alloc(*h, ITEMS) == hipSuccess && s.ready() && g_live == fixed + split);
    CHECK(s.rows_cap == hdsm::CMAX_DUO && s.items_cap == 4096 && s.sub_slots_n == 4 && s.pool_cap == 12);
    bool zero = true;
    for (int i = 0; i < 2 * 3; ++i) zero = zero && s.d_split.get()[i] == 0;
    for (int i = 0; i < 8; ++i) zero = zero && s.d_rec_count.get()[i] == 0;
    CHECK(zero);
    s.d_sub_scratch.get()[12 * 16 - 1] = 1.0, s.d_slot_busy.get()[11] = 1;
  }
  CHECK(g_live == 0);
  {  // a full life: fixed part, split state, scratch that grows three times, the pinned output block — and the end
    std::unique_ptr<Handle> h = small_handle();
    const long s0 = g_syncs;
    CHECK(h->alloc_fixed() == hipSuccess && h->sub.alloc(*h, ITEMS) == hipSuccess);
    for (size_t count : {4u, 40u, 400u}) {
      CHECK(h->stage.planes.ensure(count, h->stream.get()) == hipSuccess);
      h->stage.planes.get()[count - 1] = 1.0;
    }
    CHECK(h->stage.out.ensure(100) == hipSuccess);
    CHECK(g_syncs == s0 + 3 && g_live == fixed + split + 2);
  }
  CHECK(g_live == 0);
}

int main() {
  {  // alloc_zeroed fills; a count of 0 still allocates one element
    DevBuf<double> a;
    CHECK(!a && a.get() == nullptr && g_live == 0);
    CHECK(a.alloc_zeroed(100) == hipSuccess && a && g_live == 1);
    bool zero = true;
    for (int i = 0; i < 100; ++i) zero = zero && a.get()[i] == 0.0;
    CHECK(zero);
    DevBuf<int64_t> z;
    CHECK(z.alloc_zeroed(0) == hipSuccess && z && z.get()[0] == 0 && g_live == 2);
    z.get()[0] = -1;  // (one whole element is there: the sanitizer watches this store)
    DevBuf<int64_t> y;
    CHECK(y.alloc(0) == hipSuccess && y && g_live == 3);
    y.get()[0] = 7;
  }
  CHECK(g_live == 0);
  {  // moves: construction takes the block, assignment over a live buffer frees the old block exactly once
    DevBuf<int32_t> a, b;
    CHECK(a.alloc(4) == hipSuccess && b.alloc(4) == hipSuccess && g_live == 2);
    int32_t* pa = a.get();
    DevBuf<int32_t> c(std::move(a));
    CHECK(c.get() == pa && !a && g_live == 2);
    b = std::move(c);
    CHECK(b.get() == pa && !c && g_live == 1);
    b = std::move(c);  // (from an empty one: releases)
    CHECK(!b && g_live == 0);
    DevBuf<int32_t>& self = b;
    CHECK(b.alloc(1) == hipSuccess);
    b = std::move(self);
    CHECK(b && g_live == 1);
  }
  CHECK(g_live == 0);
  {  // grow by reallocating (stage_box), reset twice, and an allocation that fails over a live block leaves the buffer empty
    DevBuf<int8_t> e;
    size_t cap = 0;
    for (size_t bytes : {16u, 8u, 64u, 64u, 1000u}) {
      if (bytes > cap) {
        cap = 0;
        CHECK(e.alloc(bytes) == hipSuccess);
        cap = bytes;
      }
      e.get()[bytes - 1] = 1;
      CHECK(g_live == 1);
    }
    CHECK(cap == 1000);
    e.reset();
    CHECK(!e && g_live == 0);
    e.reset();
    CHECK(!e && g_live == 0);
    CHECK(e.alloc(3) == hipSuccess && g_live == 1);
    g_fail_in = 1;
    CHECK(e.alloc(5) == hipErrorOutOfMemory && !e && g_live == 0 && g_fail_in == 0);
    g_fail_in = 1;
    CHECK(e.alloc_zeroed(5) == hipErrorOutOfMemory && !e && g_live == 0);
  }
  for (int k = 1; k <= 6; ++k) {  // the k-th of the six allocations fails: the error comes back and nothing stays allocated
    Owner* o = reinterpret_cast<Owner*>(1);
    g_fail_in = k;
    CHECK(create(&o) == hipErrorOutOfMemory);
    CHECK(o == nullptr && g_live == 0);
    g_fail_in = 0;
  }
  {  // none fails: six blocks, and with the timing on 8 + 2 + 2 events; delete releases all of them
    Owner* o = nullptr;
    CHECK(create(&o) == hipSuccess && o != nullptr && g_live == 6);
    if (o) {
      CHECK(o->d_y.get()[0] == 0 && o->g.d_a.get()[1] == 0.0 && !o->ev[0]);
      for (hdsm_mem::DevEvent& e : o->ev) CHECK(e.create() == hipSuccess);
      CHECK(o->timed.create() == hipSuccess && g_live == 16);
      hipEvent_t first = o->ev[0].get();
      CHECK(o->ev[0].create() == hipSuccess && o->ev[0].get() == first && g_live == 16);  // (created once)
      hdsm_mem::DevEvent moved(std::move(o->ev[1]));
      CHECK(moved && !o->ev[1] && g_live == 16);
      o->ev[2] = std::move(moved);
      CHECK(!moved && g_live == 15);
      delete o;
    }
    CHECK(g_live == 0);
  }
  {  // the interval: refuses (and leaves the value alone) until both records of a round are in
    hdsm_mem::TimedInterval t;
    float ms = -1.0f;
    CHECK(t.ms(&ms) != hipSuccess && ms == -1.0f && g_event_calls == 0);
    CHECK(t.create() == hipSuccess && g_live == 2);
    CHECK(t.ms(&ms) != hipSuccess && ms == -1.0f);
    CHECK(t.record_start(nullptr) == hipSuccess && !t.valid);
    CHECK(t.ms(&ms) != hipSuccess && ms == -1.0f && g_event_calls == 1);
    CHECK(t.record_stop(nullptr) == hipSuccess && t.valid);
    CHECK(t.ms(&ms) == hipSuccess && ms == 0.25f && g_event_calls == 4);
    t.valid = false;
    ms = -1.0f;
    CHECK(t.ms(&ms) != hipSuccess && ms == -1.0f && g_event_calls == 4);
  }
  {  // the first error wins
    hdsm_mem::FirstError ok;
    CHECK(ok.ok());
    ok(hipSuccess), ok(hipErrorInvalidValue), ok(hipErrorOutOfMemory), ok(hipSuccess);
    CHECK(!ok.ok() && ok.e == hipErrorInvalidValue);
  }
  CHECK(g_live == 0);
  check_new_owners();
  check_handle();
  std::printf(g_failed ? "%d check(s) failed\n" : "device_mem: all checks held\n", g_failed);
  return g_failed ? 1 : 0;
}
