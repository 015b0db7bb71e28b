// rccl_stub.cpp -- a TEST-ONLY stand-in for RCCL, so that the one-process-per-device step of the product
// (flagstat_multi.hip: K1 + K2, then ONE ncclAllReduce(uint64[32], sum)) can run at world sizes 2..16 on ONE GPU.
// Real RCCL refuses two ranks on one device, and at one rank it does nothing for an in-place all-reduce; this
// library takes its place through the product's existing knob FLAGSTATS_HIP_RCCL=<path of this file's .so>.
// ncclGetVersion reports 1, so nothing that ran on it can be taken for a result with RCCL.  It says nothing about
// RCCL itself, xGMI or any timing: it checks the product's call sequence, stream ordering and buffer re-use.
//
// Ranks are PROCESSES.  They meet in one POSIX shared-memory segment whose name travels in the 128-byte id:
//   id       = "RCCLSTUB" + the segment's name (NUL-terminated)
//   segment  = header (world, who joined, who left, sticky error) + a ring of kSlots collective slots; the collective
//              with sequence number s uses slot s % kSlots: every rank writes its contribution there, and every rank
//              adds all contributions up itself, in rank order (plain uint64 addition, wrapping modulo 2^64).
// Collectives of one communicator are matched by a sequence number taken at the call, whichever stream it names.
//
// The device path of ncclAllReduce returns at once.  On the caller's stream it queues
//   1. a copy of the contribution into page-locked host memory,
//   2. a host function that only PUBLISHES it (sets a flag; it never waits for anybody),
//   3. hipStreamWaitValue64 on a page-locked word, which holds the stream,
//   4. a copy of the result from page-locked host memory into the receive buffer.
// A helper thread of the communicator takes the collectives in sequence order: it waits for the published
// contribution, exchanges through the segment, writes the sum and then the word of step 3.  No thread that the HIP
// runtime shares between streams ever waits for another rank.  Where hipStreamWaitValue64 is not available
// (hipDeviceAttributeCanUseStreamWaitValue == 0, or RCCL_STUB_NO_WAIT_VALUE=1) step 3 is dropped and the host function
// of step 2 blocks until the helper has the result (every wait bounded): safe as long as each process issues its
// collectives in stream order.
//
// Every wait is bounded (30 s; RCCL_STUB_TIMEOUT_S overrides).  When one runs out, or a rank is seen to have left,
// the stub sets a sticky error in the segment, delivers all-ones as the result, prints one line to stderr, and every
// later call of any rank on that communicator returns ncclSystemError.
//
// rccl_stub_host_allreduce(comm, inout, count) is the same exchange, synchronous and without HIP; ncclGetUniqueId,
// ncclCommInitRank, ncclCommCount and ncclCommDestroy do not touch HIP either, so the protocol is testable without a GPU.
#include <fcntl.h>
#include <sched.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace {

constexpr int kMaxRanks = 16;
constexpr int kMaxCount = 32;
constexpr uint64_t kSlots = 64;
constexpr uint64_t kMagic = 0x3142555453434352ull;  // "RCCSTUB1"
constexpr char kIdTag[8] = {'R', 'C', 'C', 'L', 'S', 'T', 'U', 'B'};
constexpr uint64_t kPoison = ~0ull;

struct Slot {
    std::atomic<uint64_t> arrived[kMaxRanks];  // s + 1 once the rank's contribution to collective s is in `data`
    uint64_t count[kMaxRanks];
    uint64_t data[kMaxRanks][kMaxCount];
};

struct Segment {
    std::atomic<uint64_t> magic;
    std::atomic<int32_t> world;     // 0 until the first rank joins
    std::atomic<int32_t> joined;    // ranks that have registered
    std::atomic<int32_t> attached;  // ranks that have the segment mapped as members; whoever brings it to 0 unlinks
    std::atomic<int32_t> error;     // sticky
    std::atomic<int32_t> taken[kMaxRanks];  // pid of the rank's process, 0 = free
    std::atomic<int32_t> left[kMaxRanks];
    std::atomic<uint64_t> done[kMaxRanks];  // collectives the rank has finished reading: slot s is free again for s + kSlots
    Slot slots[kSlots];
};
static_assert(std::atomic<uint64_t>::is_always_lock_free && std::atomic<int32_t>::is_always_lock_free, "shared atomics");

// page-locked memory of one collective in flight on a stream
struct Entry {
    uint64_t contrib[kMaxCount];
    uint64_t result[kMaxCount];
    uint64_t release;  // hipStreamWaitValue64 waits for 1 here
    std::atomic<int> published;
    std::atomic<int> finished;  // the helper is done with it (the blocking host function waits for this)
    hipEvent_t passed;          // recorded behind step 4: the stream no longer needs the entry
    double timeout_s;
};

struct Op {
    uint64_t seq = 0;
    size_t count = 0;
    Entry* entry = nullptr;      // device path
    uint64_t* host = nullptr;    // host path: in and out
    bool host_done = false;
    bool host_failed = false;
};

struct Comm {
    uint64_t tag = kMagic;
    Segment* seg = nullptr;
    char name[128] = "";
    int rank = -1, world = 0;
    double timeout_s = 30.0;
    std::mutex mu;  // sequence numbers, the queue, the entries
    std::condition_variable cv;
    std::deque<Op*> queue;
    uint64_t next_seq = 0;
    bool stop = false;
    std::atomic<int> said{0};
    std::thread helper;
    // device path, made at the first ncclAllReduce
    bool device_ready = false;
    bool wait_value = false;
    std::vector<Entry*> free_entries;
    std::deque<Entry*> busy_entries;
    std::vector<void*> chunks;
};

std::mutex g_live_mu;
std::vector<Comm*> g_live;  // for the exit handler: a process that exits with a communicator counts as having left

double now_s()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return static_cast<double>(ts.tv_sec) + 1e-9 * static_cast<double>(ts.tv_nsec);
}

// One turn of a polling loop that began at `since`: the first 200 us give the CPU away without sleeping (a collective
// among ranks that are all there costs microseconds, not a timer tick), later turns sleep 50 us.
void nap(double since)
{
    if (now_s() - since < 200e-6) {
        sched_yield();
        return;
    }
    timespec ts = {0, 50 * 1000};
    nanosleep(&ts, nullptr);
}

double timeout_from_env()
{
    const char* s = std::getenv("RCCL_STUB_TIMEOUT_S");
    if (s && *s) {
        const double v = std::atof(s);
        if (v > 0) return v;
    }
    return 30.0;
}

// poisons the communicator; one line per process and communicator
void fail_comm(Comm* c, const char* what, uint64_t seq)
{
    c->seg->error.store(1);
    if (c->said.exchange(1) == 0)
        std::fprintf(stderr, "rccl_stub: rank %d of %d (%s): %s at collective %llu; the communicator is poisoned\n", c->rank, c->world,
                     c->name, what, static_cast<unsigned long long>(seq));
}

bool valid(const Comm* c) { return c && c->tag == kMagic && c->seg; }

// The exchange of one collective; returns false (and has poisoned the communicator) when a wait ran out.
bool exchange(Comm* c, uint64_t seq, const uint64_t* in, size_t count, uint64_t* out)
{
    Segment* g = c->seg;
    Slot& slot = g->slots[seq % kSlots];
    const double began = now_s(), deadline = began + c->timeout_s;
    auto gone = [&](int r) { return g->left[r].load(std::memory_order_acquire) != 0; };
    // the slot's previous user (seq - kSlots) must have been read by every rank
    if (seq >= kSlots) {
        for (int r = 0; r < c->world; ++r) {
            while (g->done[r].load(std::memory_order_acquire) + kSlots <= seq) {
                if (g->error.load()) return false;
                if (gone(r) || now_s() > deadline) {
                    fail_comm(c, gone(r) ? "a rank has left" : "timed out waiting for a slow rank", seq);
                    return false;
                }
                nap(began);
            }
        }
    }
    if (g->error.load()) return false;
    std::memcpy(slot.data[c->rank], in, count * sizeof(uint64_t));
    slot.count[c->rank] = count;
    slot.arrived[c->rank].store(seq + 1, std::memory_order_release);
    for (int r = 0; r < c->world; ++r) {
        while (slot.arrived[r].load(std::memory_order_acquire) != seq + 1) {
            if (g->error.load()) return false;
            if (gone(r) || now_s() > deadline) {
                fail_comm(c, gone(r) ? "a rank has left" : "timed out waiting for a rank", seq);
                return false;
            }
            nap(began);
        }
        if (slot.count[r] != count) {
            fail_comm(c, "the ranks disagree on the count", seq);
            return false;
        }
    }
    uint64_t sum[kMaxCount];
    for (size_t k = 0; k < count; ++k) sum[k] = 0;
    for (int r = 0; r < c->world; ++r)
        for (size_t k = 0; k < count; ++k) sum[k] += slot.data[r][k];
    std::memcpy(out, sum, count * sizeof(uint64_t));
    g->done[c->rank].store(seq + 1, std::memory_order_release);
    return true;
}

void helper_main(Comm* c)
{
    for (;;) {
        Op* op = nullptr;
        {
            std::unique_lock<std::mutex> lk(c->mu);
            c->cv.wait(lk, [&] { return c->stop || !c->queue.empty(); });
            if (c->queue.empty()) return;  // stop, and nothing left to finish
            op = c->queue.front();
            c->queue.pop_front();
        }
        uint64_t out[kMaxCount];
        bool ok = c->seg->error.load() == 0;
        if (op->entry) {
            Entry* e = op->entry;
            const double began = now_s(), deadline = began + c->timeout_s;
            while (ok && !e->published.load(std::memory_order_acquire)) {  // this process's own stream has to get there
                if (now_s() > deadline) {
                    fail_comm(c, "timed out waiting for this rank's own stream", op->seq);
                    ok = false;
                }
                nap(began);
            }
            ok = ok && exchange(c, op->seq, e->contrib, op->count, out);
            if (!ok) {
                c->seg->error.store(1);
                for (size_t k = 0; k < op->count; ++k) out[k] = kPoison;
            }
            std::memcpy(e->result, out, op->count * sizeof(uint64_t));
            __atomic_store_n(&e->release, 1ull, __ATOMIC_RELEASE);  // lets the stream go on to the copy of the result
            e->finished.store(1, std::memory_order_release);
            delete op;
        } else {
            ok = ok && exchange(c, op->seq, op->host, op->count, out);
            if (!ok) {
                c->seg->error.store(1);
                for (size_t k = 0; k < op->count; ++k) out[k] = kPoison;
            }
            std::memcpy(op->host, out, op->count * sizeof(uint64_t));
            std::lock_guard<std::mutex> lk(c->mu);
            op->host_failed = !ok;
            op->host_done = true;
            c->cv.notify_all();
        }
    }
}

// step 2 of the device path: publish, and only where the stream cannot be held by a wait-value, wait for the helper
void publish_cb(void* p)
{
    Entry* e = static_cast<Entry*>(p);
    e->published.store(1, std::memory_order_release);
}

void publish_and_wait_cb(void* p)
{
    Entry* e = static_cast<Entry*>(p);
    e->published.store(1, std::memory_order_release);
    const double began = now_s(), deadline = began + 3.0 * e->timeout_s + 5.0;  // the helper's own waits are bounded; this is the backstop
    while (!e->finished.load(std::memory_order_acquire)) {
        if (now_s() > deadline) {
            for (int k = 0; k < kMaxCount; ++k) e->result[k] = kPoison;
            std::fprintf(stderr, "rccl_stub: a host function gave up waiting for the helper thread\n");
            return;
        }
        nap(began);
    }
}

bool device_setup(Comm* c, hipStream_t stream)
{
    if (c->device_ready) return true;
    int dev = 0, can = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess) {
        (void)hipGetLastError();
        can = 0;
    }
    const char* no = std::getenv("RCCL_STUB_NO_WAIT_VALUE");
    c->wait_value = can != 0 && !(no && *no && *no != '0');
    if (c->wait_value) {
        // the attribute says yes: try one wait that is already satisfied, so that a runtime that refuses page-locked memory
        // here is found out before a collective depends on it
        void* mem = nullptr;
        if (hipHostMalloc(&mem, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return false;
        c->chunks.push_back(mem);
        uint64_t* word = static_cast<uint64_t*>(mem);
        __atomic_store_n(word, 1ull, __ATOMIC_RELEASE);
        if (hipStreamWaitValue64(stream, word, 1, hipStreamWaitValueEq, ~0ull) != hipSuccess) {
            (void)hipGetLastError();
            c->wait_value = false;
        }
    }
    c->device_ready = true;
    return true;
}

Entry* take_entry(Comm* c)
{
    // entries whose stream has passed the copy of the result are free again; nothing here waits
    while (!c->busy_entries.empty() && c->busy_entries.front()->finished.load() &&
           hipEventQuery(c->busy_entries.front()->passed) == hipSuccess) {
        c->free_entries.push_back(c->busy_entries.front());
        c->busy_entries.pop_front();
    }
    (void)hipGetLastError();  // hipErrorNotReady of the query above is no error
    if (c->free_entries.empty()) {
        constexpr int kChunk = 64;
        void* mem = nullptr;
        if (hipHostMalloc(&mem, kChunk * sizeof(Entry), hipHostMallocDefault) != hipSuccess) return nullptr;
        c->chunks.push_back(mem);
        Entry* es = static_cast<Entry*>(mem);
        for (int i = 0; i < kChunk; ++i) {
            new (&es[i]) Entry();
            es[i].passed = nullptr;
            if (hipEventCreateWithFlags(&es[i].passed, hipEventDisableTiming) != hipSuccess) return nullptr;
            c->free_entries.push_back(&es[i]);
        }
    }
    Entry* e = c->free_entries.back();
    c->free_entries.pop_back();
    e->release = 0;
    e->published.store(0);
    e->finished.store(0);
    e->timeout_s = c->timeout_s;
    return e;
}

void leave(Comm* c)
{
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->stop = true;
        c->cv.notify_all();
    }
    if (c->helper.joinable()) c->helper.join();  // finishes what is queued first: every wait in there is bounded
    Segment* g = c->seg;
    g->left[c->rank].store(1, std::memory_order_release);
    if (g->attached.fetch_sub(1) == 1) shm_unlink(c->name);
}

struct AtExit {
    ~AtExit()
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (Comm* c : g_live) {
            // the process ends with a live communicator: the others must not wait for it, and the segment must not stay behind
            c->seg->left[c->rank].store(1, std::memory_order_release);
            if (c->seg->attached.fetch_sub(1) == 1) shm_unlink(c->name);
            if (c->helper.joinable()) c->helper.detach();
        }
        g_live.clear();
    }
} g_at_exit;

}  // namespace

extern "C" {

ncclResult_t ncclGetVersion(int* version)
{
    if (!version) return ncclInvalidArgument;
    *version = 1;
    return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
        case ncclSuccess: return "no error (rccl_stub)";
        case ncclSystemError: return "unhandled system error (rccl_stub: a rank was lost, a wait ran out, or shared memory failed)";
        case ncclInvalidArgument: return "invalid argument (rccl_stub takes ncclUint64, ncclSum, count <= 32)";
        case ncclInvalidUsage: return "invalid usage (rccl_stub)";
        default: return "error (rccl_stub)";
    }
}

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    if (!id) return ncclInvalidArgument;
    static std::atomic<unsigned> counter{0};
    std::memset(id, 0, sizeof *id);
    char name[96];
    for (int attempt = 0; attempt < 16; ++attempt) {
        std::snprintf(name, sizeof name, "/rcclstub-%d-%u-%llx", static_cast<int>(getpid()), counter.fetch_add(1),
                      static_cast<unsigned long long>(now_s() * 1e9));
        const int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0) continue;
        if (ftruncate(fd, sizeof(Segment)) != 0) {
            close(fd);
            shm_unlink(name);
            return ncclSystemError;
        }
        void* p = mmap(nullptr, sizeof(Segment), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        if (p == MAP_FAILED) {
            shm_unlink(name);
            return ncclSystemError;
        }
        static_cast<Segment*>(p)->magic.store(kMagic, std::memory_order_release);  // the rest is zero: a fresh segment
        munmap(p, sizeof(Segment));
        std::memcpy(id->internal, kIdTag, sizeof kIdTag);
        std::snprintf(id->internal + sizeof kIdTag, sizeof id->internal - sizeof kIdTag, "%s", name);
        return ncclSuccess;
    }
    return ncclSystemError;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank)
{
    if (!comm || nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    if (std::memcmp(id.internal, kIdTag, sizeof kIdTag) != 0 || id.internal[sizeof id.internal - 1] != 0) return ncclInvalidArgument;
    const char* name = id.internal + sizeof kIdTag;
    const int fd = shm_open(name, O_RDWR, 0600);
    if (fd < 0) return ncclSystemError;
    struct stat st;
    if (fstat(fd, &st) != 0 || static_cast<size_t>(st.st_size) != sizeof(Segment)) {
        close(fd);
        return ncclSystemError;
    }
    void* p = mmap(nullptr, sizeof(Segment), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) return ncclSystemError;
    Segment* g = static_cast<Segment*>(p);
    auto refuse = [&](ncclResult_t r) {
        munmap(p, sizeof(Segment));
        return r;
    };
    if (g->magic.load(std::memory_order_acquire) != kMagic) return refuse(ncclInvalidArgument);
    if (g->error.load()) return refuse(ncclSystemError);
    int32_t world = 0;
    if (!g->world.compare_exchange_strong(world, nranks) && world != nranks) {
        g->error.store(1);  // the ranks disagree on the world: nobody can finish on this communicator
        std::fprintf(stderr, "rccl_stub: rank %d says %d ranks, another said %d (%s)\n", rank, nranks, world, name);
        return refuse(ncclInvalidArgument);
    }
    int32_t nobody = 0;
    if (!g->taken[rank].compare_exchange_strong(nobody, static_cast<int32_t>(getpid()))) {
        g->error.store(1);
        std::fprintf(stderr, "rccl_stub: rank %d of %s is taken twice\n", rank, name);
        return refuse(ncclInvalidArgument);
    }
    Comm* c = new Comm();
    c->seg = g;
    std::snprintf(c->name, sizeof c->name, "%s", name);
    c->rank = rank;
    c->world = nranks;
    c->timeout_s = timeout_from_env();
    g->attached.fetch_add(1);
    g->joined.fetch_add(1);
    // like the real call: return only when everybody is here
    const double began = now_s(), deadline = began + c->timeout_s;
    while (g->joined.load(std::memory_order_acquire) < nranks && !g->error.load()) {
        if (now_s() > deadline) {
            fail_comm(c, "timed out waiting for all ranks to join", 0);
            break;
        }
        nap(began);
    }
    if (g->error.load()) {
        g->left[rank].store(1, std::memory_order_release);
        if (g->attached.fetch_sub(1) == 1) shm_unlink(c->name);
        c->tag = 0;
        delete c;
        return refuse(ncclSystemError);
    }
    c->helper = std::thread(helper_main, c);
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(c);
    }
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}

ncclResult_t ncclCommCount(const ncclComm_t comm, int* count)
{
    const Comm* c = reinterpret_cast<const Comm*>(comm);
    if (!valid(c) || !count) return ncclInvalidArgument;
    if (c->seg->error.load()) return ncclSystemError;
    *count = c->seg->world.load();
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!valid(c)) return ncclInvalidArgument;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (size_t i = 0; i < g_live.size(); ++i)
            if (g_live[i] == c) g_live.erase(g_live.begin() + static_cast<long>(i));
    }
    leave(c);
    const bool bad = c->seg->error.load() != 0;
    if (c->device_ready) {
        // the caller destroys a communicator after its streams have drained, as with the real library
        for (Entry* e : c->free_entries) (void)hipEventDestroy(e->passed);
        for (Entry* e : c->busy_entries) (void)hipEventDestroy(e->passed);
        for (void* m : c->chunks) (void)hipHostFree(m);
    }
    munmap(c->seg, sizeof(Segment));
    c->seg = nullptr;
    c->tag = 0;
    delete c;
    return bad ? ncclSystemError : ncclSuccess;
}

ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!valid(c) || !sendbuff || !recvbuff || count > kMaxCount || datatype != ncclUint64 || op != ncclSum) return ncclInvalidArgument;
    if (c->seg->error.load()) return ncclSystemError;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!device_setup(c, stream)) return ncclSystemError;
    Entry* e = take_entry(c);
    if (!e) return ncclSystemError;
    const size_t bytes = count * sizeof(uint64_t);
    if (bytes && hipMemcpyAsync(e->contrib, sendbuff, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) {
        c->free_entries.push_back(e);
        return ncclSystemError;
    }
    if (hipLaunchHostFunc(stream, c->wait_value ? publish_cb : publish_and_wait_cb, e) != hipSuccess) {
        c->free_entries.push_back(e);
        return ncclSystemError;
    }
    // from here on the collective has a sequence number and the helper will finish it, whatever the stream calls below say
    Op* o = new Op();
    o->seq = c->next_seq++;
    o->count = count;
    o->entry = e;
    c->queue.push_back(o);
    c->busy_entries.push_back(e);
    c->cv.notify_all();
    hipError_t err = hipSuccess;
    if (c->wait_value) err = hipStreamWaitValue64(stream, &e->release, 1, hipStreamWaitValueEq, ~0ull);
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(recvbuff, e->result, bytes, hipMemcpyHostToDevice, stream);
    if (err == hipSuccess) err = hipEventRecord(e->passed, stream);
    if (err != hipSuccess) {
        c->seg->error.store(1);
        std::fprintf(stderr, "rccl_stub: rank %d: %s while queueing collective %llu\n", c->rank, hipGetErrorString(err),
                     static_cast<unsigned long long>(o->seq));
        return ncclSystemError;
    }
    return ncclSuccess;
}

// stub only: the same exchange, synchronous, on host memory; no HIP call
ncclResult_t rccl_stub_host_allreduce(ncclComm_t comm, uint64_t* inout, size_t count)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!valid(c) || !inout || count > kMaxCount) return ncclInvalidArgument;
    if (c->seg->error.load()) return ncclSystemError;
    Op o;
    o.count = count;
    o.host = inout;
    std::unique_lock<std::mutex> lk(c->mu);
    o.seq = c->next_seq++;
    c->queue.push_back(&o);
    c->cv.notify_all();
    c->cv.wait(lk, [&] { return o.host_done; });  // the helper's waits are bounded, so this one is
    return o.host_failed ? ncclSystemError : ncclSuccess;
}

// stub only: 1 if collectives of this communicator hold their stream with hipStreamWaitValue64, 0 if with a blocking host
// function, -1 before the first ncclAllReduce
int rccl_stub_uses_wait_value(ncclComm_t comm)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!valid(c)) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->device_ready ? (c->wait_value ? 1 : 0) : -1;
}

// stub only, for the tests' own precondition: hold `stream` the way a collective that waits for a rank does (a
// hipStreamWaitValue64 on a fresh page-locked word); rccl_stub_release lets it go and frees the word once the stream has
// passed.  NULL where the wait-value operation is not available.  The caller releases every hold it makes.
void* rccl_stub_hold_stream(hipStream_t stream)
{
    int dev = 0, can = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess || !can) {
        (void)hipGetLastError();
        return nullptr;
    }
    void* mem = nullptr;
    if (hipHostMalloc(&mem, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return nullptr;
    __atomic_store_n(static_cast<uint64_t*>(mem), 0ull, __ATOMIC_RELEASE);
    if (hipStreamWaitValue64(stream, mem, 1, hipStreamWaitValueEq, ~0ull) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(mem);
        return nullptr;
    }
    return mem;
}

void rccl_stub_release(void* hold, hipStream_t stream)
{
    if (!hold) return;
    __atomic_store_n(static_cast<uint64_t*>(hold), 1ull, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(stream);
    (void)hipHostFree(hold);
}

}  // extern "C"
