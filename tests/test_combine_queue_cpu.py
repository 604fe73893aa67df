"""combine.h (the combining queue and the slot pool behind the prepared MSM handle, the NTT handle and the single-blob
c-kzg calls) on the CPU, under ThreadSanitizer and under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
host program (its own main, nothing preloaded, no HIP) that includes only combine.h.  Everything is checked with
counters, nothing by timing.

Queue: 16 and then 64 threads make 2000 requests each, keys from three values, with max_leaders = 3, batch_max = 32,
gather_min = 6, gather_us = 60; again with gather_us = 0; again with max_leaders = 1.  run writes f(payload) into each
request of its batch and yields.  Every request is served exactly once with its own result; every batch is, in queue
order, the front request and what is queued behind it under the same key, up to batch_max (so the order within a key is
kept); never more than max_leaders runs at once; no lane index is held by two runs at once; at the end nobody leads and
nothing is pending.  The same again, shorter, with requests that keep the empty side_work of the base (the MSM's and the
NTT's).  side_work is counted per request: every request gets at least one call, always on its caller's own
thread (a call from another thread is a race ThreadSanitizer reports), and none while the run that was passed in with
that request — its caller leading — is in progress.  That a waiting caller's side_work overlaps the batch another
leader runs for it is the design (host work beside the GPU's) and is not excluded.

Pool: 64 threads hold a slot across a barrier on a chunked pool of 48: exactly 48 distinct slots that do not overlap,
from chunks of 4, 4, 8, 16, 16 slots (five alloc calls), 16 callers without one; after release all 48 can be taken
again without another alloc; the destructor frees five chunks.  All at once: one alloc of 48 slots.  An alloc that fails
(the first, the third) is the last one tried; later acquires give the slots that are left or none; nothing leaks
(AddressSanitizer's leak check at exit)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "combine.h"
using namespace kzgamd;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #c); \
            std::_Exit(1);                                                \
        }                                                                 \
    } while (0)

static uint64_t f(uint64_t x) { return x * 0x9E3779B97F4A7C15ull + 12345; }

struct Plain : CombineRequest {  // like the MSM's and the NTT's requests: CombineRequest's empty side_work()
    static constexpr bool HAS_SIDE_WORK = false;
    int key = 0;
    uint64_t payload = 0, result = 0;
    int served = 0, side_calls = 0;
    bool own_run = false;  // its caller is inside the run it passed in
};
struct Sided : Plain {  // like the c-kzg proof requests
    static constexpr bool HAS_SIDE_WORK = true;
    void side_work() {
        CHECK(!own_run);
        ++side_calls;
    }
};

struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int waiting = 0, generation = 0;
    const int n;
    explicit Barrier(int n_) : n(n_) {}
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        const int g = generation;
        if (++waiting == n) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return generation != g; });
        }
    }
};

template <class Req>
static void queue_case(int threads, int iters, int max_leaders, int gather_us) {
    CombineQueue<Req> q;
    q.max_leaders = max_leaders;
    q.batch_max = 32;
    q.gather_min = 6;
    q.gather_us = gather_us;
    std::atomic<int> running{0}, peak{0};
    std::atomic<bool> lane_held[64];
    for (auto& l : lane_held) l = false;
    std::atomic<uint64_t> served{0}, batches{0};
    Barrier gate(threads);
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t)
        ts.emplace_back([&, t] {
            gate.wait();
            uint64_t s = 0x1234567 + (uint64_t)t * 0x9E3779B9;
            std::vector<Req*> expected;  // what the batch of this thread's next run must be
            for (int it = 0; it < iters; ++it) {
                s ^= s << 13, s ^= s >> 7, s ^= s << 17;
                Req me;
                me.key = (int)(s % 3);
                me.payload = s;
                combined_call(
                    q, me,
                    [&](const Req& front, const Req& r) {  // under q.mu, in queue order, the front first
                        if (&front == &r) {
                            CHECK(q.pending.front() == &front);
                            expected.clear();
                            for (Req* p : q.pending)
                                if (p->key == front.key && expected.size() < q.batch_max) expected.push_back(p);
                        }
                        return front.key == r.key;
                    },
                    [&](const std::vector<Req*>& batch, int lane) {
                        me.own_run = true;
                        CHECK(!batch.empty() && batch.size() <= q.batch_max);
                        CHECK(batch == expected);
                        CHECK(lane >= 0 && lane < max_leaders);
                        CHECK(!lane_held[lane].exchange(true));
                        const int now = ++running;
                        CHECK(now <= max_leaders);
                        int p = peak.load();
                        while (p < now && !peak.compare_exchange_weak(p, now)) {
                        }
                        for (Req* r : batch) {
                            CHECK(r->key == batch[0]->key);
                            r->result = f(r->payload);
                            ++r->served;
                        }
                        std::this_thread::yield();
                        served += batch.size();
                        ++batches;
                        --running;
                        CHECK(lane_held[lane].exchange(false));
                        me.own_run = false;
                    });
                CHECK(me.done && me.served == 1 && me.result == f(me.payload));
                if (Req::HAS_SIDE_WORK) CHECK(me.side_calls >= 1 && me.side_calls <= 2);
            }
        });
    for (auto& th : ts) th.join();
    CHECK(served == (uint64_t)threads * iters);
    CHECK(peak >= 1 && peak <= max_leaders);
    CHECK(q.leaders == 0 && q.lanes_taken == 0 && q.pending.empty());
    std::printf("queue side_work=%d threads=%d leaders=%d gather_us=%d: %llu requests in %llu batches, peak %d\n", (int)Req::HAS_SIDE_WORK, threads, max_leaders,
                gather_us, (unsigned long long)served.load(), (unsigned long long)batches.load(), peak.load());
}

struct AllocStats {
    int calls = 0, frees = 0, fail_at = 0;  // fail_at: the call (from 1) that fails; 0 = none
    std::vector<size_t> sizes;
};
struct CountingAlloc {
    AllocStats* st;
    void* alloc(size_t bytes) {
        st->sizes.push_back(bytes);
        if (++st->calls == st->fail_at) return nullptr;
        return std::malloc(bytes);
    }
    void free(void* p) {
        ++st->frees;
        std::free(p);
    }
};

static void pool_chunked() {
    const size_t SB = 96;
    const int THREADS = 64, MAX = 48;
    AllocStats st;
    {
        SlotPool<CountingAlloc> pool(SB, MAX, SlotGrowth::Chunked, CountingAlloc{&st});
        CHECK(st.calls == 0);
        std::vector<unsigned char*> got(THREADS, nullptr);
        Barrier gate(THREADS);
        std::vector<std::thread> ts;
        for (int t = 0; t < THREADS; ++t)
            ts.emplace_back([&, t] {
                gate.wait();
                got[t] = pool.acquire();
                if (got[t]) std::memset(got[t], t, SB);
                gate.wait();  // every thread holds what it got
                if (got[t])
                    for (size_t i = 0; i < SB; ++i) CHECK(got[t][i] == (unsigned char)t);
                gate.wait();
                pool.release(got[t]);  // ignores the NULLs
            });
        for (auto& th : ts) th.join();
        std::vector<unsigned char*> held;
        for (auto* p : got)
            if (p) held.push_back(p);
        CHECK((int)held.size() == MAX);
        std::sort(held.begin(), held.end());
        for (size_t i = 1; i < held.size(); ++i) CHECK(held[i] - held[i - 1] >= (ptrdiff_t)SB);
        CHECK(st.calls == 5);
        CHECK((st.sizes == std::vector<size_t>{4 * SB, 4 * SB, 8 * SB, 16 * SB, 16 * SB}));
        std::vector<unsigned char*> again;
        for (int i = 0; i < MAX; ++i) {
            again.push_back(pool.acquire());
            CHECK(again.back() != nullptr);
        }
        CHECK(pool.acquire() == nullptr);
        std::sort(again.begin(), again.end());
        CHECK(again == held);
        for (auto* p : again) pool.release(p);
        CHECK(st.calls == 5 && st.frees == 0);
    }
    CHECK(st.frees == 5);
}

static void pool_all_at_once() {
    const size_t SB = 128;
    AllocStats st;
    {
        SlotPool<CountingAlloc> pool(SB, 48, SlotGrowth::AllAtOnce, CountingAlloc{&st});
        std::vector<unsigned char*> held;
        for (int i = 0; i < 48; ++i) {
            held.push_back(pool.acquire());
            CHECK(held.back() != nullptr);
            std::memset(held.back(), i, SB);
        }
        CHECK(pool.acquire() == nullptr);
        CHECK(st.calls == 1 && st.sizes[0] == 48 * SB);
        std::sort(held.begin(), held.end());
        for (size_t i = 1; i < held.size(); ++i) CHECK(held[i] - held[i - 1] >= (ptrdiff_t)SB);
        for (auto* p : held) pool.release(p);
    }
    CHECK(st.calls == 1 && st.frees == 1);
}

static void pool_failures() {
    for (SlotGrowth g : {SlotGrowth::Chunked, SlotGrowth::AllAtOnce}) {  // the first alloc fails
        AllocStats st;
        st.fail_at = 1;
        {
            SlotPool<CountingAlloc> pool(64, 48, g, CountingAlloc{&st});
            for (int i = 0; i < 3; ++i) CHECK(pool.acquire() == nullptr);
            pool.release(nullptr);
            CHECK(st.calls == 1);
        }
        CHECK(st.calls == 1 && st.frees == 0);
    }
    AllocStats st;  // the third fails: 4 + 4 slots are all there will be
    st.fail_at = 3;
    {
        SlotPool<CountingAlloc> pool(64, 48, SlotGrowth::Chunked, CountingAlloc{&st});
        std::vector<unsigned char*> held;
        for (int i = 0; i < 8; ++i) {
            held.push_back(pool.acquire());
            CHECK(held.back() != nullptr);
        }
        CHECK(st.calls == 2);
        CHECK(pool.acquire() == nullptr);
        CHECK(st.calls == 3);
        CHECK(pool.acquire() == nullptr);
        pool.release(held.back());
        CHECK(pool.acquire() == held.back());
        CHECK(pool.acquire() == nullptr);
        CHECK(st.calls == 3);
        for (auto* p : held) pool.release(p);
    }
    CHECK(st.calls == 3 && st.frees == 2);
}

int main() {
    for (int threads : {16, 64}) {
        queue_case<Sided>(threads, 2000, 3, 60);
        queue_case<Sided>(threads, 2000, 3, 0);
        queue_case<Sided>(threads, 2000, 1, 60);
    }
    for (int threads : {16, 64}) {  // the same without side work, at a quarter of the length
        queue_case<Plain>(threads, 500, 3, 60);
        queue_case<Plain>(threads, 500, 3, 0);
        queue_case<Plain>(threads, 500, 1, 60);
    }
    pool_chunked();
    pool_all_at_once();
    pool_failures();
    std::printf("done\n");
    return 0;
}
'''


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_queue_and_pool_under_a_sanitizer(tmp_path, sanitizer):
    # clang first: the ThreadSanitizer runtime of g++ 11 does not know pthread_cond_clockwait (what wait_until on the
    # steady clock calls) and reports the mutex as locked twice
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    src = tmp_path / "combine_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "combine_check"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitizer]
    if sanitizer != "thread":
        cmd.append("-fno-sanitize-recover=all")
    cmd += ["-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)]
    # whether the sanitizer can be used at all is decided on an empty program with the same flags: only that may skip.
    # Every failure to build or run the real program fails the test.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(cmd[:-3] + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("done"), (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
