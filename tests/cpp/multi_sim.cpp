// A simulated multi-GPU node for sift-gpu_amd/csrc/multi.hip, and its driver.
//
// multi.hip has no kernel and is layered on the public C ABI only, so it builds
// unchanged with the host compiler.  This program defines every symbol it leaves
// undefined -- 17 of the HIP runtime, 8 of RCCL, 9 of the C ABI -- links with it
// and runs the step / gather / flush pipeline at 1, 2, 3, 4 and 8 devices on the
// CPU.  The HIP and RCCL headers are included for their types only; no ROCm
// library is linked.
//
// The node
//   memory    device and pinned allocations are exact-size heap blocks tagged with
//             the device that was current, fresh ones filled with 0xA5; every
//             access is looked up, so a copy that leaves its buffer or touches
//             another device's memory fails (and an address sanitizer build sees
//             it too).
//   streams   an enqueue only appends an op (fake detect, async copy, event
//             record, wait, the stream's part of a p2p group) to the stream's
//             queue.  Nothing runs at enqueue time.
//   events    hipStreamWaitEvent binds to the event's most recent record at the
//             time of the call (HIP's rule); a never-recorded event is no wait;
//             recording an event on a stream of another device is an error.
//   RCCL      the sends and receives between ncclGroupStart and ncclGroupEnd are
//             one op per participating stream, which runs when every such stream
//             has it at its head; sends and receives pair per (sender rank,
//             receiver rank) in posting order; an unpaired op or a pair of
//             different byte sizes fails the run.  A call that fails inside a
//             group makes ncclGroupEnd drop the whole group and return the error,
//             as NCCL does.  A comm's rank is its index in ncclCommInitAll's list.
//   schedule  a host wait (hipEventSynchronize, hipStreamSynchronize, the fake
//             sift_sync, stream / context destruction) drives the scheduler until
//             its target completes; which runnable op runs next is the schedule:
//             FIFO with everything eager, demand-only (the dependency closure of
//             the target), compute eager + gather demand-only, gather eager +
//             compute demand-only, and seeded random orders.  A blocking hipMemcpy
//             runs on the null stream, which does not order against the
//             non-blocking streams used here: it gives eager streams their turn
//             and copies.  No runnable op with the target incomplete is a deadlock.
//   hazards   every op carries the byte ranges it reads and writes.  When an op
//             runs while an op the host enqueued EARLIER is still pending and the
//             two conflict (one writes what the other touches), the run fails:
//             FIFO order is one legal execution, so any schedule that reorders a
//             conflicting pair computes something else.  This is what sees a
//             missing "slot free again" wait: through the public interface its
//             wrong bytes land only in a gathered step the caller did not collect
//             (collecting a step waits for its gather before the next step can be
//             enqueued), so a byte comparison alone cannot.
//   contexts  sift_ctx_create records device and sub-batch size and owns a stream;
//             sift_detect_compute_batch_masked records its arguments and enqueues
//             a detect op which, when it runs, writes offsets, records and
//             descriptors that depend on (unit, step, image, record) and poisons
//             the rest of the slot.
//   accounts  every allocation, stream, event, comm and context must be released
//             exactly once; a leak, a double release or a use after release fails.
//   faults    the j-th fallible call into the node can be made to fail.  The
//             release calls (hipFree, hipHostFree, the stream, event, comm and
//             context destroys), whose results multi.hip ignores, always
//             succeed and are not counted.
//
// The driver runs every schedule over n x S x gather_desc (and SIFT_MULTI_SELF_P2P
// at n = 1, 2), twice: collecting every step, and collecting only after the flush.
// Then the capacity error path and the fault-injection sweeps.
//
//   multi_sim [--n LIST]     (device counts to run, default 1,2,3,4,8)
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sift_hip.h"

// ---------------------------------------------------------------------------
// the node's objects: the opaque handle types of the three headers, defined here
// ---------------------------------------------------------------------------
struct Access {
  const char* p;
  size_t n;
  bool write;
};
struct Group;
struct Op {
  enum Kind { DETECT, COPY, RECORD, WAIT, GROUP } kind = RECORD;
  long long gseq = 0;  // host enqueue order over all streams
  ihipStream_t* wstream = nullptr;  // WAIT: the record it is bound to (null: none)
  long long wseq = -1;
  void* dst = nullptr;  // COPY
  const void* src = nullptr;
  size_t bytes = 0;
  sift_ctx* ctx = nullptr;  // DETECT
  int call = -1;
  Group* group = nullptr;  // GROUP
  std::vector<Access> acc;
};
struct ihipStream_t {
  int id = 0, dev = 0;
  bool gather = false;  // created by multi.hip itself; a context's stream is a compute stream
  bool live = true;
  std::deque<Op> q;
  long long enq = 0, done = 0;  // ops enqueued / completed; the head op has index `done`
};
struct ihipEvent_t {
  int id = 0, dev = 0;
  bool live = true;
  ihipStream_t* rstream = nullptr;  // most recent record
  long long rseq = -1;
};
struct ncclComm {
  int rank = 0, dev = 0;
  bool live = true;
};
struct P2p {
  bool send;
  char* buf;
  size_t bytes;
  int rank, peer;
  ihipStream_t* stream;
};
struct Group {
  int id = 0;
  std::vector<P2p> ops;
  std::vector<ihipStream_t*> streams;
  std::vector<std::pair<int, int>> pairs;  // (send, receive) indices into ops
  std::vector<Access> acc;
};
struct DetectCall {
  long long step;
  const float* imgs;
  int batch, rows, cols;
  size_t row_stride, img_stride;
  const uint8_t* masks;
  size_t mask_row_stride, mask_img_stride;
  sift_keypoint* kpts;
  float* desc;
  int cap;
  int* offs;
};
struct sift_ctx {
  int unit = 0, dev = 0, max_batch = 0;
  unsigned create_flags = 0, flags = 0;
  int octaves = 5, max_features = 0;
  int n_set_flags = 0, n_set_octaves = 0, n_set_max_features = 0;
  ihipStream_t* stream = nullptr;
  bool live = true;
  int sticky = 0;
  std::vector<DetectCall> calls;
  std::string err;
};

namespace {

constexpr int kDevices = 8;
constexpr unsigned char kPoison = 0xA5;

enum Sched { FIFO, DEMAND, COMPUTE_EAGER, GATHER_EAGER, RANDOM };
const char* const kSchedName[] = {"fifo-eager", "demand-only", "compute-eager/gather-demand",
                                  "gather-eager/compute-demand", "random"};

// The data the fake detect writes: the configuration of a run and, from it, the
// images of every unit and step and the records of every image.
struct Config {
  int n = 1, S_req = 1, gather_desc = 0;
  bool self_p2p = false;
  bool collect_every_step = true;
  int max_batch = 5, kp_cap = 61, steps = 6;
  int over_step = -1, over_unit = -1;  // the unit that emits cap + 1 records (error path)
  int phase = 0;                       // where in the rotation of counts step 0 starts

  int S() const { return std::max(1, std::min(S_req ? S_req : 2, max_batch)); }
  int U() const { return n * S(); }
  int cap() const { return (kp_cap + S() - 1) / S(); }
  int sub_batch() const { return (max_batch + S() - 1) / S(); }
  // per-device image counts: every step another rotation of full, none, one
  // (below S, so a sub-batch is empty), and two uneven counts
  int count(long long t, int i) const {
    static const int table[5] = {5, 0, 1, 4, 3};
    return std::min(table[(i + t + phase) % 5], max_batch);
  }
  // sub-batch j of S takes the contiguous images [floor(j c / S), floor((j + 1) c / S))
  void slice(long long t, int u, int* first, int* c) const {
    const int cnt = count(t, u / S()), j = u % S();
    *first = (int)((long long)j * cnt / S());
    *c = (int)((long long)(j + 1) * cnt / S()) - *first;
  }
  // the last unit of the first device with a full count fills its slot exactly
  int exact_unit(long long t) const {
    for (int i = 0; i < n; ++i)
      if (count(t, i) == max_batch) return i * S() + S() - 1;
    return -1;
  }
};

uint32_t mix(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  uint32_t h = 0x9E3779B9u;
  const uint32_t v[4] = {a, b, c, d};
  for (int i = 0; i < 4; ++i) {
    h ^= v[i] + 0x85EBCA6Bu + (h << 6) + (h >> 2);
    h *= 0xC2B2AE35u;
    h ^= h >> 15;
  }
  return h;
}

int rec_count(const Config& c, long long t, int u, int b) {
  int first, cnt;
  c.slice(t, u, &first, &cnt);
  const int per = c.cap() / c.sub_batch();
  auto plain = [&](int bb) {
    if (mix(u, (uint32_t)t, bb, 2) % 3 == 0) return 0;
    return (int)(mix(u, (uint32_t)t, bb, 1) % (uint32_t)(per + 1));
  };
  if (b == cnt - 1 && (u == c.exact_unit(t) || (u == c.over_unit && t == c.over_step))) {
    int before = 0;
    for (int bb = 0; bb < b; ++bb) before += plain(bb);
    return c.cap() + (u == c.over_unit && t == c.over_step ? 1 : 0) - before;
  }
  return plain(b);
}

sift_keypoint make_kp(long long t, int u, int b, int r) {
  sift_keypoint k;
  k.x = (float)u;
  k.y = (float)t;
  k.size = (float)b;
  k.angle = (float)r;
  k.response = (float)(mix(u, (uint32_t)t, b, r) & 0xffff);
  k.octave = (int32_t)mix(u, (uint32_t)t, b, r + 1000);
  k.class_id = (int32_t)(((u * 131 + (int)t) * 131 + b) * 131 + r);
  return k;
}

// descriptor element e of a record: a 24-bit integer, exact in a float
uint32_t desc_seed(long long t, int u, int b, int r) { return mix(u, (uint32_t)t, b, r + 5000); }
float make_desc(uint32_t seed, int e) { return (float)((seed + (uint32_t)e * 0x9E3779B1u) >> 8); }

struct Alloc {
  char* p;
  size_t n;
  int dev;
  bool pinned;
};

struct Node {
  int cur_dev = 0;
  long long gseq = 0;
  std::map<const char*, Alloc> mem;
  std::vector<std::unique_ptr<ihipStream_t>> streams;
  std::vector<std::unique_ptr<ihipEvent_t>> events;
  std::vector<std::unique_ptr<ncclComm>> comms;
  std::vector<std::unique_ptr<sift_ctx>> ctxs;
  std::vector<std::unique_ptr<Group>> groups;
  Group* open_group = nullptr;
  int group_depth = 0;
  bool group_error = false;
  long long step = 0;  // the driver's step index, stamped on every detect call
  Sched sched = FIFO;
  uint64_t rng = 1;
  long long calls = 0, fail_at = -1;  // fault injection: the fail_at-th fallible call fails
  Config cfg;
  long long ops_run = 0;
  long long p2p_posted = 0;      // sends and receives accepted
  long long groups_dropped = 0;  // failed groups that held posted ops
  ~Node() {
    for (auto& kv : mem) free(kv.second.p);
  }
};

Node* N = nullptr;
std::string g_where;  // configuration, schedule and seed of the current run

[[noreturn]] void die(const char* fmt, ...) {
  fflush(stderr);
  printf("FAIL [%s]: ", g_where.c_str());
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  printf("\n");
  fflush(stdout);
  _exit(1);
}

#define REQUIRE(cond, ...) \
  do {                     \
    if (!(cond)) die(__VA_ARGS__); \
  } while (0)

bool inject() { return N->calls++ == N->fail_at; }

uint32_t rnd() {
  N->rng = N->rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(N->rng >> 33);
}

// ---- memory ---------------------------------------------------------------
const Alloc& find_alloc(const void* ptr, size_t bytes, const char* what) {
  const char* p = static_cast<const char*>(ptr);
  auto it = N->mem.upper_bound(p);
  REQUIRE(it != N->mem.begin(), "%s: %p is in no live allocation", what, ptr);
  --it;
  const Alloc& a = it->second;
  REQUIRE(p + bytes <= a.p + a.n, "%s: %zu bytes at offset %zu leave a buffer of %zu bytes (or it was released)", what,
          bytes, (size_t)(p - a.p), a.n);
  return a;
}

const Alloc& find_device(const void* ptr, size_t bytes, int dev, const char* what) {
  const Alloc& a = find_alloc(ptr, bytes, what);
  REQUIRE(!a.pinned, "%s: host memory where device memory is expected", what);
  REQUIRE(a.dev == dev, "%s: memory of device %d used on device %d", what, a.dev, dev);
  return a;
}

void* node_alloc(size_t bytes, bool pinned) {
  char* p = static_cast<char*>(malloc(bytes ? bytes : 1));
  REQUIRE(p, "host allocation of %zu bytes failed", bytes);
  memset(p, kPoison, bytes);
  N->mem[p] = Alloc{p, bytes, N->cur_dev, pinned};
  return p;
}

bool overlap(const Access& a, const Access& b) { return a.p < b.p + b.n && b.p < a.p + a.n; }
bool conflict(const std::vector<Access>& x, const std::vector<Access>& y) {
  for (const Access& a : x)
    for (const Access& b : y)
      if ((a.write || b.write) && overlap(a, b)) return true;
  return false;
}
const std::vector<Access>& accesses(const Op& o) { return o.kind == Op::GROUP ? o.group->acc : o.acc; }

std::string describe(const Op& o, const ihipStream_t* s) {
  static const char* const names[] = {"detect", "copy", "record", "wait", "p2p group"};
  char buf[160];
  if (o.kind == Op::WAIT)
    snprintf(buf, sizeof buf, "wait #%lld on %s stream %d (device %d) for op %lld of stream %d", o.gseq,
             s->gather ? "gather" : "compute", s->id, s->dev, o.wseq, o.wstream ? o.wstream->id : -1);
  else if (o.kind == Op::GROUP)
    snprintf(buf, sizeof buf, "p2p group %d #%lld on gather stream %d (device %d)", o.group->id, o.gseq, s->id, s->dev);
  else
    snprintf(buf, sizeof buf, "%s #%lld on %s stream %d (device %d)", names[o.kind], o.gseq,
             s->gather ? "gather" : "compute", s->id, s->dev);
  return buf;
}

void release_alloc(void* ptr, bool pinned, const char* what) {
  if (!ptr) return;
  auto it = N->mem.find(static_cast<const char*>(ptr));
  REQUIRE(it != N->mem.end(), "%s: %p is not a live allocation (double release?)", what, ptr);
  REQUIRE(it->second.pinned == pinned, "%s: wrong kind of memory", what);
  const std::vector<Access> whole{Access{it->second.p, it->second.n, true}};
  for (auto& s : N->streams)
    for (const Op& o : s->q)
      REQUIRE(!conflict(whole, accesses(o)), "%s: released while %s is still queued", what, describe(o, s.get()).c_str());
  free(it->second.p);
  N->mem.erase(it);
}

// ---- handles --------------------------------------------------------------
ihipStream_t* use(ihipStream_t* s, const char* what) {
  REQUIRE(s, "%s: the null stream is not modelled", what);
  REQUIRE(s->live, "%s: stream %d used after release", what, s->id);
  return s;
}
ihipEvent_t* use(ihipEvent_t* e, const char* what) {
  REQUIRE(e, "%s: null event", what);
  REQUIRE(e->live, "%s: event %d used after release", what, e->id);
  return e;
}
ncclComm* use(ncclComm* c, const char* what) {
  REQUIRE(c, "%s: null communicator", what);
  REQUIRE(c->live, "%s: communicator of rank %d used after release", what, c->rank);
  return c;
}
sift_ctx* use(sift_ctx* c, const char* what) {
  REQUIRE(c, "%s: null context", what);
  REQUIRE(c->live, "%s: context of unit %d used after release", what, c->unit);
  return c;
}
const sift_ctx* use(const sift_ctx* c, const char* what) { return use(const_cast<sift_ctx*>(c), what); }

ihipStream_t* new_stream(int dev, bool gather) {
  N->streams.emplace_back(new ihipStream_t);
  ihipStream_t* s = N->streams.back().get();
  s->id = (int)N->streams.size() - 1;
  s->dev = dev;
  s->gather = gather;
  return s;
}

long long enqueue(ihipStream_t* s, Op o) {
  o.gseq = N->gseq++;
  s->q.push_back(std::move(o));
  return s->enq++;
}

// ---- the scheduler --------------------------------------------------------
bool satisfied(const Op& o) { return !o.wstream || o.wstream->done > o.wseq; }

bool runnable(const ihipStream_t* s) {
  if (s->q.empty()) return false;
  const Op& o = s->q.front();
  if (o.kind == Op::WAIT) return satisfied(o);
  if (o.kind == Op::GROUP) {
    for (const ihipStream_t* t : o.group->streams)
      if (t->q.empty() || t->q.front().group != o.group) return false;
  }
  return true;
}

[[noreturn]] void deadlock(const ihipStream_t* target, long long tseq) {
  fflush(stderr);
  printf("FAIL [%s]: deadlock: the host waits for op %lld of stream %d and no op is runnable; queue heads:\n",
         g_where.c_str(), tseq, target ? target->id : -1);
  for (auto& s : N->streams)
    if (s->live && !s->q.empty())
      printf("  stream %d: %zu queued, head: %s\n", s->id, s->q.size(), describe(s->q.front(), s.get()).c_str());
  fflush(stdout);
  _exit(1);
}

void run_detect(const Op& o) {
  const Config& c = N->cfg;
  const sift_ctx* ctx = o.ctx;
  const DetectCall& d = ctx->calls[o.call];
  int total = 0;
  d.offs[0] = 0;
  for (int b = 0; b < d.batch; ++b) {
    const int k = rec_count(c, d.step, ctx->unit, b);
    for (int r = 0; r < k; ++r, ++total) {
      if (total >= d.cap) continue;  // only the first cap rows are written; the offsets keep the true total
      d.kpts[total] = make_kp(d.step, ctx->unit, b, r);
      const uint32_t seed = desc_seed(d.step, ctx->unit, b, r);
      for (int e = 0; e < SIFT_DESC_LEN; ++e) d.desc[(size_t)total * SIFT_DESC_LEN + e] = make_desc(seed, e);
    }
    d.offs[b + 1] = total;
  }
  const int kept = std::min(total, d.cap);
  memset(reinterpret_cast<char*>(d.kpts + kept), kPoison, sizeof(sift_keypoint) * (size_t)(d.cap - kept));
  memset(reinterpret_cast<char*>(d.desc + (size_t)kept * SIFT_DESC_LEN), kPoison,
         sizeof(float) * SIFT_DESC_LEN * (size_t)(d.cap - kept));
  if (total > d.cap) o.ctx->sticky = SIFT_E_CAPACITY;
}

void run_head(ihipStream_t* s) {
  const Op& o = s->q.front();
  // an op the host enqueued earlier, still pending, that conflicts with this one
  for (auto& t : N->streams)
    for (const Op& y : t->q) {
      if (accesses(o).empty()) break;
      if (&y == &o || (o.kind == Op::GROUP && y.group == o.group)) continue;
      if (y.gseq < o.gseq && conflict(accesses(o), accesses(y)))
        die("hazard: %s ran while the earlier-enqueued %s, which touches the same bytes, was still pending",
            describe(o, s).c_str(), describe(y, t.get()).c_str());
    }
  ++N->ops_run;
  switch (o.kind) {
    case Op::DETECT: run_detect(o); break;
    case Op::COPY: memcpy(o.dst, o.src, o.bytes); break;
    case Op::RECORD:
    case Op::WAIT: break;
    case Op::GROUP: {
      Group* g = o.group;
      for (auto& pr : g->pairs) memcpy(g->ops[pr.second].buf, g->ops[pr.first].buf, g->ops[pr.first].bytes);
      for (ihipStream_t* t : g->streams) {
        if (t == s) continue;
        t->q.pop_front();
        ++t->done;
      }
      break;
    }
  }
  s->q.pop_front();
  ++s->done;
}

bool eager(const ihipStream_t* s) {
  switch (N->sched) {
    case FIFO: return true;
    case COMPUTE_EAGER: return !s->gather;
    case GATHER_EAGER: return s->gather;
    default: return false;
  }
}

// Drives the node until op tseq of stream target is complete (no target: eager
// streams get their turn, nothing is demanded).
void drive(ihipStream_t* target, long long tseq) {
  auto complete = [&] { return !target || target->done > tseq; };
  if (N->sched == RANDOM) {
    for (;;) {
      std::vector<ihipStream_t*> cand;
      for (auto& s : N->streams)
        if (s->live && runnable(s.get())) cand.push_back(s.get());
      if (complete()) {
        if (cand.empty() || rnd() % 4 == 0) return;
      } else if (cand.empty()) {
        deadlock(target, tseq);
      }
      run_head(cand[rnd() % cand.size()]);
    }
  }
  for (;;) {
    for (;;) {
      ihipStream_t* best = nullptr;
      for (auto& s : N->streams)
        if (s->live && eager(s.get()) && runnable(s.get()) && (!best || s->q.front().gseq < best->q.front().gseq))
          best = s.get();
      if (!best) break;
      run_head(best);
    }
    if (complete()) return;
    // the dependency closure of the target: only queue heads can run
    std::vector<ihipStream_t*> need{target};
    auto add = [&](ihipStream_t* s) {
      if (std::find(need.begin(), need.end(), s) == need.end()) need.push_back(s);
    };
    for (size_t k = 0; k < need.size(); ++k) {
      ihipStream_t* s = need[k];
      if (s->q.empty()) continue;
      const Op& o = s->q.front();
      if (o.kind == Op::WAIT && !satisfied(o)) add(o.wstream);
      if (o.kind == Op::GROUP)
        for (ihipStream_t* t : o.group->streams) add(t);
    }
    ihipStream_t* best = nullptr;
    for (ihipStream_t* s : need)
      if (runnable(s) && (!best || s->q.front().gseq < best->q.front().gseq)) best = s;
    if (!best) deadlock(target, tseq);
    run_head(best);
  }
}

void drain(ihipStream_t* s) { drive(s, s->enq - 1); }

size_t nccl_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8:
    case ncclUint8: return 1;
    case ncclFloat16:
    case ncclBfloat16: return 2;
    case ncclInt32:
    case ncclUint32:
    case ncclFloat32: return 4;
    case ncclInt64:
    case ncclUint64:
    case ncclFloat64: return 8;
    default: die("ncclSend/ncclRecv: datatype %d is not modelled", (int)t);
  }
}

void close_group() {
  Group* g = N->open_group;
  N->open_group = nullptr;
  const bool failed = N->group_error;
  N->group_error = false;
  if (failed && !g->ops.empty()) ++N->groups_dropped;
  if (failed || g->ops.empty()) return;  // a failed group launches nothing
  const int ranks = (int)N->comms.size();
  for (int a = 0; a < ranks; ++a)
    for (int b = 0; b < ranks; ++b) {
      std::vector<int> sends, recvs;
      for (int k = 0; k < (int)g->ops.size(); ++k) {
        const P2p& o = g->ops[k];
        if (o.send && o.rank == a && o.peer == b) sends.push_back(k);
        if (!o.send && o.rank == b && o.peer == a) recvs.push_back(k);
      }
      REQUIRE(sends.size() == recvs.size(),
              "unpaired p2p op: rank %d posts %zu sends to rank %d, which posts %zu receives from it", a, sends.size(),
              b, recvs.size());
      for (size_t k = 0; k < sends.size(); ++k) {
        REQUIRE(g->ops[sends[k]].bytes == g->ops[recvs[k]].bytes,
                "p2p size mismatch: send %zu of rank %d to rank %d is %zu bytes, its receive %zu bytes", k, a, b,
                g->ops[sends[k]].bytes, g->ops[recvs[k]].bytes);
        g->pairs.emplace_back(sends[k], recvs[k]);
      }
    }
  REQUIRE(g->pairs.size() * 2 == g->ops.size(), "unpaired p2p op: a peer rank outside the communicator");
  for (const P2p& o : g->ops) {
    g->acc.push_back(Access{o.buf, o.bytes, !o.send});
    if (std::find(g->streams.begin(), g->streams.end(), o.stream) == g->streams.end()) g->streams.push_back(o.stream);
  }
  const long long gseq = N->gseq++;
  for (ihipStream_t* s : g->streams) {
    Op op;
    op.kind = Op::GROUP;
    op.group = g;
    op.gseq = gseq;
    s->q.push_back(op);
    ++s->enq;
  }
}

ncclResult_t post_p2p(bool send, const void* buf, size_t count, ncclDataType_t type, int peer, ncclComm* comm,
                      ihipStream_t* stream) {
  const char* what = send ? "ncclSend" : "ncclRecv";
  if (inject()) {
    if (N->open_group) N->group_error = true;
    return ncclInternalError;
  }
  use(comm, what);
  use(stream, what);
  REQUIRE(stream->dev == comm->dev, "%s: communicator of device %d with a stream of device %d", what, comm->dev,
          stream->dev);
  REQUIRE(peer >= 0 && peer < (int)N->comms.size(), "%s: peer %d outside the communicator", what, peer);
  const size_t bytes = count * nccl_size(type);
  find_device(buf, bytes, comm->dev, what);
  const bool single = !N->open_group;
  if (single) {
    N->groups.emplace_back(new Group);
    N->open_group = N->groups.back().get();
    N->open_group->id = (int)N->groups.size() - 1;
  }
  ++N->p2p_posted;
  N->open_group->ops.push_back(
      P2p{send, const_cast<char*>(static_cast<const char*>(buf)), bytes, comm->rank, peer, stream});
  if (single) close_group();
  return ncclSuccess;
}

}  // namespace

// ---------------------------------------------------------------------------
// HIP runtime
// ---------------------------------------------------------------------------
extern "C" {

hipError_t hipSetDevice(int d) {
  if (inject()) return hipErrorUnknown;
  if (d < 0 || d >= kDevices) return hipErrorInvalidDevice;
  N->cur_dev = d;
  return hipSuccess;
}

hipError_t hipGetDeviceCount(int* count) {
  if (inject()) return hipErrorUnknown;
  *count = kDevices;
  return hipSuccess;
}

const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorInvalidHandle: return "invalid resource handle";
    case hipErrorInvalidValue: return "invalid argument";
    default: return "injected failure";
  }
}

hipError_t hipMalloc(void** ptr, size_t size) {
  if (inject()) return hipErrorOutOfMemory;
  *ptr = node_alloc(size, false);
  return hipSuccess;
}

hipError_t hipFree(void* ptr) {
  release_alloc(ptr, false, "hipFree");
  return hipSuccess;
}

hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
  if (inject()) return hipErrorOutOfMemory;
  *ptr = node_alloc(size, true);
  return hipSuccess;
}

hipError_t hipHostFree(void* ptr) {
  release_alloc(ptr, true, "hipHostFree");
  return hipSuccess;
}

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (inject()) return hipErrorUnknown;
  REQUIRE(kind == hipMemcpyDeviceToHost, "hipMemcpy: only device-to-host copies are modelled");
  find_device(src, bytes, N->cur_dev, "hipMemcpy source");
  drive(nullptr, 0);
  const std::vector<Access> rd{Access{static_cast<const char*>(src), bytes, false}};
  for (auto& s : N->streams)
    for (const Op& o : s->q)
      REQUIRE(!conflict(rd, accesses(o)), "hazard: a blocking hipMemcpy reads bytes that the pending %s writes",
              describe(o, s.get()).c_str());
  memcpy(dst, src, bytes);
  return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  if (inject()) return hipErrorUnknown;
  use(stream, "hipMemcpyAsync");
  REQUIRE(kind == hipMemcpyDeviceToDevice || kind == hipMemcpyDeviceToHost,
          "hipMemcpyAsync: copy kind %d is not modelled", (int)kind);
  find_device(src, bytes, stream->dev, "hipMemcpyAsync source");
  if (kind == hipMemcpyDeviceToDevice)
    find_device(dst, bytes, stream->dev, "hipMemcpyAsync destination");
  else
    REQUIRE(find_alloc(dst, bytes, "hipMemcpyAsync destination").pinned,
            "hipMemcpyAsync destination: device memory in a device-to-host copy");
  Op op;
  op.kind = Op::COPY;
  op.dst = dst;
  op.src = src;
  op.bytes = bytes;
  op.acc = {Access{static_cast<const char*>(src), bytes, false}, Access{static_cast<const char*>(dst), bytes, true}};
  enqueue(stream, std::move(op));
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int flags) {
  if (inject()) return hipErrorUnknown;
  REQUIRE(flags == hipStreamNonBlocking, "hipStreamCreateWithFlags: only non-blocking streams are modelled");
  *stream = new_stream(N->cur_dev, true);
  return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t stream) {
  use(stream, "hipStreamDestroy");
  drain(stream);  // HIP lets the queued work finish
  stream->live = false;
  return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t stream) {
  if (inject()) return hipErrorUnknown;
  drain(use(stream, "hipStreamSynchronize"));
  return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int) {
  if (inject()) return hipErrorUnknown;
  use(stream, "hipStreamWaitEvent");
  use(event, "hipStreamWaitEvent");
  Op op;
  op.kind = Op::WAIT;
  op.wstream = event->rstream;  // the most recent record, now; never recorded: no wait
  op.wseq = event->rseq;
  enqueue(stream, std::move(op));
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) {
  if (inject()) return hipErrorUnknown;
  N->events.emplace_back(new ihipEvent_t);
  ihipEvent_t* e = N->events.back().get();
  e->id = (int)N->events.size() - 1;
  e->dev = N->cur_dev;
  *event = e;
  return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event) {
  use(event, "hipEventDestroy")->live = false;
  return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
  if (inject()) return hipErrorUnknown;
  use(event, "hipEventRecord");
  use(stream, "hipEventRecord");
  if (event->dev != stream->dev) return hipErrorInvalidHandle;  // as HIP: event and stream of different devices
  Op op;
  op.kind = Op::RECORD;
  event->rstream = stream;
  event->rseq = enqueue(stream, std::move(op));
  return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t event) {
  if (inject()) return hipErrorUnknown;
  use(event, "hipEventSynchronize");
  if (event->rstream) {
    REQUIRE(event->rstream->live, "hipEventSynchronize: the stream of the event's record was released");
    drive(event->rstream, event->rseq);
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// RCCL
// ---------------------------------------------------------------------------
ncclResult_t ncclGetVersion(int* version) {
  if (inject()) return ncclInternalError;
  *version = NCCL_VERSION_CODE;
  return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t r) { return r == ncclSuccess ? "no error" : "injected failure"; }

ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist) {
  if (inject()) return ncclSystemError;
  REQUIRE(N->comms.empty(), "ncclCommInitAll: called twice in one run");
  for (int i = 0; i < ndev; ++i) {
    REQUIRE(devlist[i] >= 0 && devlist[i] < kDevices, "ncclCommInitAll: device %d", devlist[i]);
    N->comms.emplace_back(new ncclComm);
    N->comms.back()->rank = i;
    N->comms.back()->dev = devlist[i];
    comm[i] = N->comms.back().get();
  }
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  use(comm, "ncclCommDestroy")->live = false;
  return ncclSuccess;
}

ncclResult_t ncclGroupStart() {
  if (inject()) return ncclInternalError;
  if (N->group_depth++ == 0) {
    N->groups.emplace_back(new Group);
    N->open_group = N->groups.back().get();
    N->open_group->id = (int)N->groups.size() - 1;
    N->group_error = false;
  }
  return ncclSuccess;
}

ncclResult_t ncclGroupEnd() {
  REQUIRE(N->group_depth > 0, "ncclGroupEnd without ncclGroupStart");
  const bool fail = inject();
  if (fail) N->group_error = true;
  if (--N->group_depth > 0) return fail ? ncclInternalError : ncclSuccess;
  const bool failed = N->group_error;
  close_group();
  return failed ? ncclInternalError : ncclSuccess;
}

ncclResult_t ncclSend(const void* buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm,
                      hipStream_t stream) {
  return post_p2p(true, buf, count, type, peer, comm, stream);
}

ncclResult_t ncclRecv(void* buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream) {
  return post_p2p(false, buf, count, type, peer, comm, stream);
}

// ---------------------------------------------------------------------------
// the C ABI's contexts
// ---------------------------------------------------------------------------
int sift_ctx_create(int device, int, int, int max_batch, unsigned flags, sift_ctx** out) {
  *out = nullptr;
  if (inject()) return SIFT_E_HIP;
  if (device < 0 || device >= kDevices || max_batch < 1) return SIFT_E_INVALID;
  N->ctxs.emplace_back(new sift_ctx);
  sift_ctx* c = N->ctxs.back().get();
  c->unit = (int)N->ctxs.size() - 1;
  c->dev = device;
  c->max_batch = max_batch;
  c->create_flags = c->flags = flags;
  c->stream = new_stream(device, false);
  N->cur_dev = device;  // the real one leaves its device current
  *out = c;
  return SIFT_OK;
}

int sift_ctx_destroy(sift_ctx* c) {
  use(c, "sift_ctx_destroy");
  use(c->stream, "sift_ctx_destroy");
  drain(c->stream);
  c->stream->live = false;
  c->live = false;
  return SIFT_OK;
}

const char* sift_last_error(const sift_ctx* c) { return use(c, "sift_last_error")->err.c_str(); }
void* sift_get_stream(sift_ctx* c) { return use(c, "sift_get_stream")->stream; }

int sift_sync(sift_ctx* c) {
  if (inject()) return SIFT_E_HIP;
  drain(use(c, "sift_sync")->stream);
  const int rc = c->sticky;
  c->sticky = 0;
  if (rc) c->err = "sticky device status";
  return rc;
}

int sift_set_flags(sift_ctx* c, unsigned flags) {
  if (inject()) return SIFT_E_HIP;
  use(c, "sift_set_flags")->flags = flags;
  ++c->n_set_flags;
  return SIFT_OK;
}

int sift_set_octaves(sift_ctx* c, int n) {
  if (inject()) return SIFT_E_HIP;
  use(c, "sift_set_octaves")->octaves = n;
  ++c->n_set_octaves;
  return SIFT_OK;
}

int sift_set_max_features(sift_ctx* c, int n) {
  if (inject()) return SIFT_E_HIP;
  ++use(c, "sift_set_max_features")->n_set_max_features;
  if (n < 0) return SIFT_E_INVALID;
  c->max_features = n;
  return SIFT_OK;
}

int sift_detect_compute_batch_masked(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols, size_t row_stride,
                                     size_t img_stride, const uint8_t* d_masks, size_t mask_row_stride,
                                     size_t mask_img_stride, sift_keypoint* d_kpts, float* d_desc, int kp_cap,
                                     int* d_img_offsets) {
  if (inject()) {
    c->err = "injected failure";
    return SIFT_E_HIP;
  }
  use(c, "sift_detect_compute_batch_masked");
  if (batch > c->max_batch) {
    c->err = "batch larger than the context was created for";
    return SIFT_E_SIZE;
  }
  REQUIRE(batch > 0 && kp_cap > 0, "detect on unit %d: batch %d, kp_cap %d", c->unit, batch, kp_cap);
  find_device(d_imgs, sizeof(float) * ((size_t)(batch - 1) * img_stride + (size_t)(rows - 1) * row_stride + cols),
              c->dev, "detect images");
  if (d_masks)
    find_device(d_masks, (size_t)(batch - 1) * mask_img_stride + (size_t)(rows - 1) * mask_row_stride + cols, c->dev,
                "detect masks");
  find_device(d_kpts, sizeof(sift_keypoint) * (size_t)kp_cap, c->dev, "detect records");
  find_device(d_desc, sizeof(float) * SIFT_DESC_LEN * (size_t)kp_cap, c->dev, "detect descriptors");
  find_device(d_img_offsets, sizeof(int) * (size_t)(batch + 1), c->dev, "detect offsets");
  c->calls.push_back(DetectCall{N->step, d_imgs, batch, rows, cols, row_stride, img_stride, d_masks, mask_row_stride,
                                mask_img_stride, d_kpts, d_desc, kp_cap, d_img_offsets});
  Op op;
  op.kind = Op::DETECT;
  op.ctx = c;
  op.call = (int)c->calls.size() - 1;
  op.acc = {Access{reinterpret_cast<const char*>(d_kpts), sizeof(sift_keypoint) * (size_t)kp_cap, true},
            Access{reinterpret_cast<const char*>(d_desc), sizeof(float) * SIFT_DESC_LEN * (size_t)kp_cap, true},
            Access{reinterpret_cast<const char*>(d_img_offsets), sizeof(int) * (size_t)(batch + 1), true}};
  enqueue(c->stream, std::move(op));
  return SIFT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// the driver
// ---------------------------------------------------------------------------
namespace {

const int kDeviceOrder[kDevices] = {5, 2, 7, 0, 3, 6, 1, 4};  // rank i is not device i
constexpr int kRows = 3, kCols = 4;
constexpr size_t kRowStride = 5, kImgStride = 17, kMaskRowStride = 6, kMaskImgStride = 19;

void fresh_node(const Config& c, Sched sched, uint64_t seed) {
  delete N;
  N = new Node;
  N->cfg = c;
  N->sched = sched;
  N->rng = seed * 0x9E3779B97F4A7C15ull + 12345;
}

void set_where(const Config& c, Sched sched, uint64_t seed, const char* what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: n=%d S=%d gather_desc=%d self_p2p=%d collect=%s schedule=%s seed=%llu", what, c.n,
           c.S_req, c.gather_desc, (int)c.self_p2p, c.collect_every_step ? "every step" : "after the flush",
           kSchedName[sched], (unsigned long long)seed);
  g_where = buf;
}

void check_released() {
  REQUIRE(N->mem.empty(), "leak: %zu allocations were not released (the first has %zu bytes on device %d)",
          N->mem.size(), N->mem.empty() ? 0 : N->mem.begin()->second.n,
          N->mem.empty() ? -1 : N->mem.begin()->second.dev);
  for (auto& s : N->streams) REQUIRE(!s->live, "leak: stream %d (device %d) was not released", s->id, s->dev);
  for (auto& e : N->events) REQUIRE(!e->live, "leak: event %d (device %d) was not released", e->id, e->dev);
  for (auto& c : N->comms) REQUIRE(!c->live, "leak: communicator of rank %d was not released", c->rank);
  for (auto& c : N->ctxs) REQUIRE(!c->live, "leak: context of unit %d was not released", c->unit);
  REQUIRE(N->group_depth == 0 && !N->open_group, "a p2p group was left open (depth %d)", N->group_depth);
}

// One multi context and the caller's side of it: images and masks on every device.
struct Run {
  Config c;
  sift_multi* m = nullptr;
  int devices[kDevices];
  float* imgs[kDevices] = {};
  uint8_t* masks[kDevices] = {};
  sift_keypoint* slot_k[2][64] = {};
  long long exp_records = 0, exp_transfers = 0;
  int exact_seen = 0;

  int create() {
    for (int i = 0; i < c.n; ++i) devices[i] = kDeviceOrder[i];
    return sift_multi_create(devices, c.n, 64, 64, c.max_batch, (c.self_p2p ? SIFT_MULTI_SELF_P2P : 0u) | SIFT_FLAG_FAST,
                             c.S_req, c.kp_cap, c.gather_desc, &m);
  }
  void alloc_inputs() {
    for (int i = 0; i < c.n; ++i) {
      N->cur_dev = devices[i];
      imgs[i] = static_cast<float*>(node_alloc(sizeof(float) * kImgStride * c.max_batch, false));
      masks[i] = static_cast<uint8_t*>(node_alloc(kMaskImgStride * c.max_batch, false));
    }
    N->cur_dev = 0;
  }
  void free_inputs() {
    for (int i = 0; i < c.n; ++i) {
      release_alloc(imgs[i], false, "driver");
      release_alloc(masks[i], false, "driver");
      imgs[i] = nullptr;
      masks[i] = nullptr;
    }
  }
  // step t: no masks, per-image masks (odd devices without), one shared mask per device
  int step(long long t) {
    N->step = t;
    int counts[kDevices];
    const float* di[kDevices];
    const uint8_t* dm[kDevices];
    for (int i = 0; i < c.n; ++i) {
      counts[i] = c.count(t, i);
      di[i] = counts[i] ? imgs[i] : nullptr;
      dm[i] = (t % 3 == 1 && i % 2 == 1) ? nullptr : masks[i];
    }
    if (t % 3 == 0) return sift_multi_step(m, di, counts, kRows, kCols, kRowStride, kImgStride);
    return sift_multi_step_masked(m, di, dm, counts, kRows, kCols, kRowStride, kImgStride, kMaskRowStride,
                                  t % 3 == 1 ? kMaskImgStride : 0);
  }
  // every context got exactly its slice of step t
  void check_calls(long long t) {
    for (int u = 0; u < c.U(); ++u) {
      const sift_ctx* x = N->ctxs[u].get();
      const int i = u / c.S();
      int first, cnt;
      c.slice(t, u, &first, &cnt);
      std::vector<const DetectCall*> mine;
      for (const DetectCall& d : x->calls)
        if (d.step == t) mine.push_back(&d);
      REQUIRE((int)mine.size() == (cnt > 0 ? 1 : 0), "wrong slice: unit %d got %zu detect calls in step %lld for %d images",
              u, mine.size(), t, cnt);
      if (!cnt) continue;
      const DetectCall& d = *mine[0];
      REQUIRE(x->dev == devices[i], "wrong slice: unit %d runs on device %d, not %d", u, x->dev, devices[i]);
      REQUIRE(d.imgs == imgs[i] + (size_t)first * kImgStride && d.batch == cnt,
              "wrong slice: unit %d step %lld got images at +%td x %d, expected +%zu x %d", u, t, d.imgs - imgs[i],
              d.batch, (size_t)first * kImgStride, cnt);
      REQUIRE(d.rows == kRows && d.cols == kCols && d.row_stride == kRowStride && d.img_stride == kImgStride,
              "wrong slice: unit %d step %lld got the image shape %d x %d, strides %zu / %zu", u, t, d.rows, d.cols,
              d.row_stride, d.img_stride);
      const uint8_t* em = nullptr;
      if (t % 3 == 1 && i % 2 == 0) em = masks[i] + (size_t)first * kMaskImgStride;
      if (t % 3 == 2) em = masks[i];
      REQUIRE(d.masks == em, "wrong slice: unit %d step %lld (first image %d) got the mask pointer %p, expected %p", u, t,
              first, (const void*)d.masks, (const void*)em);
      if (em)
        REQUIRE(d.mask_row_stride == kMaskRowStride && d.mask_img_stride == (t % 3 == 1 ? kMaskImgStride : 0),
                "wrong slice: unit %d step %lld got the mask strides %zu / %zu", u, t, d.mask_row_stride,
                d.mask_img_stride);
      REQUIRE(d.cap == c.cap(), "unit %d step %lld: kp_cap %d, expected %d", u, t, d.cap, c.cap());
      // exact-size result slots on the unit's device, alternating between two
      const Alloc& ak = find_device(d.kpts, sizeof(sift_keypoint) * (size_t)d.cap, x->dev, "record slot");
      const Alloc& ad = find_device(d.desc, sizeof(float) * SIFT_DESC_LEN * (size_t)d.cap, x->dev, "descriptor slot");
      REQUIRE(ak.p == (const char*)d.kpts && ak.n == sizeof(sift_keypoint) * (size_t)d.cap &&
                  ad.p == (const char*)d.desc && ad.n == sizeof(float) * SIFT_DESC_LEN * (size_t)d.cap,
              "unit %d step %lld: the result slots are not allocations of cap records", u, t);
      sift_keypoint*& mineslot = slot_k[t & 1][u];
      REQUIRE(!mineslot || mineslot == d.kpts, "unit %d step %lld: the slot of this parity changed", u, t);
      mineslot = d.kpts;
      REQUIRE(slot_k[0][u] != slot_k[1][u], "unit %d step %lld: both slots are one buffer", u, t);
    }
  }
  // what the gather of step t adds to the totals
  void account(long long t) {
    for (int u = 0; u < c.U(); ++u) {
      int first, cnt, total = 0;
      c.slice(t, u, &first, &cnt);
      for (int b = 0; b < cnt; ++b) total += rec_count(c, t, u, b);
      exp_records += total;
      if (total > 0 && (u >= c.S() || c.self_p2p)) exp_transfers += c.gather_desc ? 2 : 1;
      if (cnt > 0 && total == c.cap()) ++exact_seen;
    }
  }
  void check_stats(long long steps) {
    long long s = -1, r = -1, x = -1;
    REQUIRE(sift_multi_stats(m, &s, &r, &x) == SIFT_OK, "sift_multi_stats failed");
    REQUIRE(s == steps && r == exp_records && x == exp_transfers,
            "wrong stats: steps %lld records %lld transfers %lld, expected %lld / %lld / %lld", s, r, x, steps,
            exp_records, exp_transfers);
  }
  // the gathered step must be step t, byte for byte
  void check_gathered(long long t) {
    std::vector<int> eoff{0};
    std::vector<sift_keypoint> ek;
    std::vector<float> ed;
    for (int u = 0; u < c.U(); ++u) {
      int first, cnt;
      c.slice(t, u, &first, &cnt);
      for (int b = 0; b < cnt; ++b) {
        const int k = rec_count(c, t, u, b);
        for (int r = 0; r < k; ++r) {
          ek.push_back(make_kp(t, u, b, r));
          const uint32_t seed = desc_seed(t, u, b, r);
          for (int e = 0; e < SIFT_DESC_LEN; ++e) ed.push_back(make_desc(seed, e));
        }
        eoff.push_back((int)ek.size());
      }
    }
    const int bt_exp = (int)eoff.size() - 1, total = (int)ek.size();
    const sift_keypoint* dk = nullptr;
    const float* dd = nullptr;
    std::vector<int> off(bt_exp + 1, -7);
    int bt = -1;
    long long step = -1;
    int rc = sift_multi_gathered(m, &dk, &dd, off.data(), bt_exp + 1, &bt, &step);
    // read rk / rd here, before anything else drives the node
    REQUIRE(rc == SIFT_OK, "sift_multi_gathered failed (%d): %s", rc, sift_multi_last_error(m));
    REQUIRE(step == t && bt == bt_exp, "gathered step %lld with %d images, expected step %lld with %d", step, bt, t,
            bt_exp);
    REQUIRE(off == eoff, "wrong offsets for step %lld", t);
    REQUIRE((dd != nullptr) == (c.gather_desc != 0), "descriptor pointer %p with gather_desc = %d", (const void*)dd,
            c.gather_desc);
    find_device(dk, sizeof(sift_keypoint) * (size_t)total, devices[0], "gathered records");
    for (int k = 0; k < total; ++k)
      REQUIRE(!memcmp(&dk[k], &ek[k], sizeof(sift_keypoint)),
              "wrong bytes: record %d of %d of gathered step %lld on device 0 (x %g y %g size %g angle %g, expected %g %g %g %g)",
              k, total, t, dk[k].x, dk[k].y, dk[k].size, dk[k].angle, ek[k].x, ek[k].y, ek[k].size, ek[k].angle);
    if (dd) {
      find_device(dd, sizeof(float) * SIFT_DESC_LEN * (size_t)total, devices[0], "gathered descriptors");
      for (int k = 0; k < total; ++k)
        REQUIRE(!memcmp(dd + (size_t)k * SIFT_DESC_LEN, ed.data() + (size_t)k * SIFT_DESC_LEN,
                        sizeof(float) * SIFT_DESC_LEN),
                "wrong bytes: descriptor %d of %d of gathered step %lld on device 0", k, total, t);
    }
    if (bt_exp > 0)
      REQUIRE(sift_multi_gathered(m, nullptr, nullptr, off.data(), bt_exp, nullptr, nullptr) == SIFT_E_CAPACITY,
              "sift_multi_gathered accepted a short offsets buffer");
    // exact-size host buffers: a copy of more than the total leaves them
    sift_keypoint* hk = static_cast<sift_keypoint*>(malloc(sizeof(sift_keypoint) * (size_t)std::max(total, 1)));
    float* hd = static_cast<float*>(malloc(sizeof(float) * SIFT_DESC_LEN * (size_t)std::max(total, 1)));
    int n_out = -1;
    rc = sift_multi_copy_gathered(m, hk, c.gather_desc ? hd : nullptr, total, &n_out);
    REQUIRE(rc == SIFT_OK && n_out == total, "sift_multi_copy_gathered: rc %d, %d records, expected %d: %s", rc, n_out,
            total, sift_multi_last_error(m));
    REQUIRE(!total || !memcmp(hk, ek.data(), sizeof(sift_keypoint) * (size_t)total),
            "wrong bytes: records of step %lld from sift_multi_copy_gathered", t);
    REQUIRE(!total || !c.gather_desc || !memcmp(hd, ed.data(), sizeof(float) * SIFT_DESC_LEN * (size_t)total),
            "wrong bytes: descriptors of step %lld from sift_multi_copy_gathered", t);
    if (total > 0) {
      REQUIRE(sift_multi_copy_gathered(m, hk, nullptr, total - 1, &n_out) == SIFT_E_CAPACITY && n_out == total,
              "sift_multi_copy_gathered accepted a short buffer");
      if (!c.gather_desc)
        REQUIRE(sift_multi_copy_gathered(m, hk, hd, total, &n_out) == SIFT_E_INVALID,
                "sift_multi_copy_gathered copied descriptors that were not gathered");
    }
    free(hk);
    free(hd);
  }
  void check_setters() {
    const int U = c.U();
    REQUIRE((int)N->ctxs.size() == U, "%zu contexts for %d units", N->ctxs.size(), U);
    for (int u = 0; u < U; ++u) {
      const sift_ctx* x = N->ctxs[u].get();
      REQUIRE(x->dev == devices[u / c.S()] && x->max_batch == c.sub_batch() && x->create_flags == SIFT_FLAG_FAST,
              "unit %d: device %d, sub-batch %d, flags %#x", u, x->dev, x->max_batch, x->create_flags);
    }
    for (int i = 0; i < c.n; ++i)
      REQUIRE(sift_multi_context(m, i) == N->ctxs[i * c.S()].get(), "sift_multi_context(%d) is not its first unit", i);
    REQUIRE(sift_multi_context(m, c.n) == nullptr && sift_multi_context(m, -1) == nullptr,
            "sift_multi_context out of range");
    REQUIRE(sift_multi_set_octaves(m, 4) == SIFT_OK && sift_multi_set_flags(m, SIFT_FLAG_NO_GRAPH) == SIFT_OK &&
                sift_multi_set_max_features(m, 7) == SIFT_OK,
            "a setter failed: %s", sift_multi_last_error(m));
    REQUIRE(sift_multi_set_max_features(m, -1) == SIFT_E_INVALID, "sift_multi_set_max_features(-1) was accepted");
    for (int u = 0; u < U; ++u) {
      const sift_ctx* x = N->ctxs[u].get();
      REQUIRE(x->octaves == 4 && x->n_set_octaves == 1, "unit %d: octaves %d after %d calls", u, x->octaves,
              x->n_set_octaves);
      REQUIRE(x->flags == SIFT_FLAG_NO_GRAPH && x->n_set_flags == 1, "unit %d: flags %#x after %d calls", u, x->flags,
              x->n_set_flags);
      REQUIRE(x->max_features == 7 && x->n_set_max_features == 1,
              "unit %d: max_features %d after %d calls (the refused -1 must reach no context)", u, x->max_features,
              x->n_set_max_features);
    }
  }
  void destroy() {
    REQUIRE(sift_multi_destroy(m) == SIFT_OK, "sift_multi_destroy failed");
    m = nullptr;
    free_inputs();
    check_released();
  }
};

void run_config(const Config& c, Sched sched, uint64_t seed) {
  set_where(c, sched, seed, "pipeline");
  fresh_node(c, sched, seed);
  Run r;
  r.c = c;
  int rc = r.create();
  REQUIRE(rc == SIFT_OK && r.m, "sift_multi_create failed (%d)", rc);
  r.alloc_inputs();
  r.check_setters();
  const sift_keypoint* dk = nullptr;
  REQUIRE(sift_multi_gathered(r.m, &dk, nullptr, nullptr, 0, nullptr, nullptr) == SIFT_E_INVALID,
          "sift_multi_gathered before any gather");
  for (long long t = 0; t < c.steps; ++t) {
    rc = r.step(t);
    REQUIRE(rc == SIFT_OK, "step %lld failed (%d): %s", t, rc, sift_multi_last_error(r.m));
    r.check_calls(t);
    if (t > 0) r.account(t - 1);
    r.check_stats(t + 1);
    if (t > 0 && c.collect_every_step) r.check_gathered(t - 1);
  }
  rc = sift_multi_flush(r.m);
  REQUIRE(rc == SIFT_OK, "flush failed (%d): %s", rc, sift_multi_last_error(r.m));
  r.account(c.steps - 1);
  r.check_stats(c.steps);
  r.check_gathered(c.steps - 1);
  REQUIRE(r.exact_seen > 0, "no unit filled its slot exactly: the driver's counts are wrong");
  REQUIRE(sift_multi_flush(r.m) == SIFT_OK, "a second flush failed: %s", sift_multi_last_error(r.m));
  r.check_gathered(c.steps - 1);
  r.destroy();
}

// A unit over cap at n = 2: the error names the device, the multi context is final.
void run_capacity(Sched sched) {
  Config c;
  c.n = 2;
  c.S_req = 2;
  c.gather_desc = 1;
  // step 2: device 0 has 1 image, device 1 has 4: unit 3 (device 1, second sub-batch) overflows
  c.over_step = 2;
  c.over_unit = 3;
  set_where(c, sched, 0, "capacity");
  fresh_node(c, sched, 0);
  Run r;
  r.c = c;
  REQUIRE(r.create() == SIFT_OK, "sift_multi_create failed");
  r.alloc_inputs();
  for (long long t = 0; t < 3; ++t) REQUIRE(r.step(t) == SIFT_OK, "step %lld failed: %s", t, sift_multi_last_error(r.m));
  const int rc = r.step(3);  // gathers step 2
  const std::string msg = sift_multi_last_error(r.m);
  const std::string dev = "device " + std::to_string(r.devices[1]) + ":";
  REQUIRE(rc == SIFT_E_CAPACITY && msg.find(dev) != std::string::npos,
          "the overflow of unit 3 gave %d \"%s\", expected SIFT_E_CAPACITY naming \"%s\"", rc, msg.c_str(), dev.c_str());
  REQUIRE(r.step(4) == SIFT_E_INVALID, "a step after the overflow was accepted");
  REQUIRE(sift_multi_flush(r.m) == SIFT_E_INVALID, "a flush after the overflow was accepted");
  r.destroy();
}

// Every fallible call of sift_multi_create fails in turn.
int sweep_create(Sched sched) {
  Config c;
  c.n = 2;
  c.S_req = 2;
  c.gather_desc = 1;
  set_where(c, sched, 0, "create, clean");
  fresh_node(c, sched, 0);
  Run clean;
  clean.c = c;
  REQUIRE(clean.create() == SIFT_OK, "sift_multi_create failed");
  const long long calls = N->calls;
  clean.alloc_inputs();
  clean.destroy();
  for (long long j = 0; j < calls; ++j) {
    set_where(c, sched, (uint64_t)j, "create, call <seed> fails");
    fresh_node(c, sched, 0);
    N->fail_at = j;
    Run r;
    r.c = c;
    const int rc = r.create();
    REQUIRE(N->calls > j, "the create made only %lld calls", N->calls);
    REQUIRE(rc != SIFT_OK && !r.m, "sift_multi_create returned %d and %p although call %lld failed", rc, (void*)r.m, j);
    check_released();
  }
  return (int)calls;
}

// Every fallible call of two steps + flush fails in turn.  The counts are {1, 4}
// and {4, 3} images on the two devices, so the second step's gather and the
// flush's both post sends, receives and descriptor pairs from device 1: the
// sweep reaches a failed call inside a group that already holds posted ops.
// The entry point that made the failing call must itself return non-zero,
// those before it succeed, and those after a failed step are refused.
int sweep_step(Sched sched) {
  Config c;
  c.n = 2;
  c.S_req = 2;
  c.gather_desc = 1;
  c.phase = 2;
  long long end[3] = {-1, -1, -1};  // the clean run's call count after each entry point
  long long dropped = 0;
  for (long long j = -1; j < end[2] || end[2] < 0; ++j) {
    set_where(c, sched, (uint64_t)j, j < 0 ? "steps + flush, clean" : "steps + flush, call <seed> fails");
    fresh_node(c, sched, 0);
    Run r;
    r.c = c;
    REQUIRE(r.create() == SIFT_OK, "sift_multi_create failed");
    r.alloc_inputs();
    N->calls = 0;
    N->fail_at = j;
    int rc[3];
    long long after[3], posted[3];
    for (int e = 0; e < 3; ++e) {
      rc[e] = e < 2 ? r.step(e) : sift_multi_flush(r.m);
      after[e] = N->calls;
      posted[e] = N->p2p_posted;
      if (j < 0) {
        REQUIRE(rc[e] == SIFT_OK, "the clean run failed: %s", sift_multi_last_error(r.m));
        if (e > 0) {
          r.account(e - 1);
          r.check_stats(2);
          r.check_gathered(e - 1);
          N->calls = after[e];  // the checks' own calls are not part of the sweep
        }
      }
    }
    if (j < 0) {
      for (int e = 0; e < 3; ++e) end[e] = after[e];
      // both gathers cross devices: records and descriptors of two units of device 1
      REQUIRE(posted[0] == 0 && posted[1] >= 4 && posted[2] >= posted[1] + 4 && posted[2] == 2 * r.exp_transfers,
              "the swept steps posted %lld / %lld / %lld p2p ops for %lld transfers: the sweep must cross devices",
              posted[0], posted[1], posted[2], r.exp_transfers);
    } else {
      const int who = j < end[0] ? 0 : j < end[1] ? 1 : 2;
      static const char* const names[3] = {"the first step", "the second step", "the flush"};
      REQUIRE(N->calls > j, "the steps and the flush made only %lld calls", N->calls);
      for (int e = 0; e < who; ++e)
        REQUIRE(rc[e] == SIFT_OK, "%s failed (%d) before the failing call %lld was made", names[e], rc[e], j);
      REQUIRE(rc[who] != SIFT_OK, "call %lld failed inside %s, which returned 0", j, names[who]);
      for (int e = who + 1; e < 3; ++e)
        REQUIRE(rc[e] == SIFT_E_INVALID, "%s failed (%d) and %s after it returned %d", names[who], rc[who], names[e],
                rc[e]);
      REQUIRE(N->group_depth == 0 && !N->open_group, "call %lld failed and left a p2p group open", j);
    }
    N->fail_at = -1;
    dropped += N->groups_dropped;
    r.destroy();
  }
  REQUIRE(dropped > 0, "no injected failure fell inside a p2p group that held posted ops");
  return (int)end[2];
}

}  // namespace

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  std::vector<int> ns{1, 2, 3, 4, 8};
  for (int a = 1; a + 1 < argc; a += 2)
    if (!strcmp(argv[a], "--n")) {
      ns.clear();
      for (const char* p = argv[a + 1]; *p;) {
        ns.push_back(atoi(p));
        while (*p && *p != ',') ++p;
        if (*p) ++p;
      }
    }
  struct Order {
    Sched sched;
    uint64_t seed;
  };
  std::vector<Order> orders{{FIFO, 0}, {DEMAND, 0}, {COMPUTE_EAGER, 0}, {GATHER_EAGER, 0}};
  for (uint64_t seed = 1; seed <= 32; ++seed) orders.push_back({RANDOM, seed});

  std::vector<Config> configs;
  for (int n : ns)
    for (int S = 1; S <= 3; ++S)
      for (int gd = 0; gd < 2; ++gd)
        for (int self = 0; self < (n <= 2 ? 2 : 1); ++self) {
          Config c;
          c.n = n;
          c.S_req = S;
          c.gather_desc = gd;
          c.self_p2p = self != 0;
          configs.push_back(c);
        }
  long long ops = 0;
  for (const Config& base : configs)
    for (const Order& o : orders)
      for (int every = 1; every >= 0; --every) {
        Config c = base;
        c.collect_every_step = every != 0;
        run_config(c, o.sched, o.seed ? o.seed * 1000 + c.n * 100 + c.S_req * 10 + c.gather_desc : 0);
        ops += N->ops_run;
      }
  int create_calls = 0, step_calls = 0;
  for (Sched s : {FIFO, DEMAND, COMPUTE_EAGER, GATHER_EAGER}) {
    if (std::find(ns.begin(), ns.end(), 2) == ns.end()) break;  // the error paths run at n = 2
    run_capacity(s);
    create_calls = sweep_create(s);
    step_calls = sweep_step(s);
  }
  delete N;
  N = nullptr;
  printf("multi sim ok: %zu configs, %zu schedules (%lld ops run; faults injected at %d create and %d steps + flush calls)\n",
         configs.size(), orders.size(), ops, create_calls, step_calls);
  return 0;
}
