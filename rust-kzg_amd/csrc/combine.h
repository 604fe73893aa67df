// Combining of concurrent host-buffer calls on one shared handle: the queue callers put their requests
// on, the loop in which up to max_leaders of them at a time run everything queued as batches, and the pool of staging
// slots a caller copies its input into on its own thread.  Three users: the prepared MSM handle (msm.hip), the NTT
// handle (ntt.hip) and the single-blob c-kzg entry points (ckzg.hip).
// Host-only and free of HIP: tests/test_combine_queue_cpu.py runs it under ThreadSanitizer and AddressSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <type_traits>
#include <vector>

namespace kzgamd {

// what combined_call needs of a request; side_work() is the part of a call that needs no GPU
struct CombineRequest {
    bool done = false;
    void side_work() {}
};

template <class Req>
struct CombineQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Req*> pending;
    int leaders = 0;
    uint64_t lanes_taken = 0;  // bit i: a leader holds lane i (max_leaders <= 64)
    // set once, when the handle is created
    int max_leaders = 1;    // batches in flight at once
    size_t batch_max = 1;   // requests per batch
    size_t gather_min = 0;  // with another batch in flight, a leader waits for this many queued requests ...
    int gather_us = 0;      // ... but at most this long (0: no wait)
};

// Queues `me` and returns once it is served.  While fewer than max_leaders callers lead and something is pending, a
// caller leads: it takes the lowest free lane index and, until its own request is served or nothing is left, takes the
// front request and everything queued behind it that is same(front, r) — in queue order, up to batch_max — and calls
// run(batch, lane) without the lock.  run must not throw: it records a failure in the requests.  A caller returns as
// soon as its own request is served; leadership passes to whoever is waiting.  A caller that does not lead calls
// me.side_work() once before it first sleeps, and every caller once more when it is served.
// Everything that can allocate (the batch's reserve, the push) happens before the request is visible to other callers:
// a bad_alloc leaves by exception with nothing queued.
template <class Req, class Same, class Run>
void combined_call(CombineQueue<Req>& q, Req& me, Same&& same, Run&& run) {
    std::vector<Req*> batch;
    batch.reserve(q.batch_max);
    // a request type that keeps CombineRequest's empty side_work() gives up the lock for nothing: it goes straight to sleep
    constexpr bool has_side_work = !std::is_same<decltype(&Req::side_work), void (CombineRequest::*)()>::value;
    const bool gathers = q.gather_us > 0 && q.gather_min > 0;
    std::unique_lock<std::mutex> lk(q.mu);
    q.pending.push_back(&me);
    // a leader gathering requests may have enough now.  Nobody else sleeps for a push (a waiting caller is woken when a
    // batch is done or a leader leaves), and a wake-up per push is not free next to a combined call of 13 us
    if (gathers) q.cv.notify_one();
    bool idled = !has_side_work;
    while (!me.done) {
        if (q.leaders < q.max_leaders && !q.pending.empty()) {
            ++q.leaders;
            int lane = 0;
            while (q.lanes_taken >> lane & 1) ++lane;  // leaders <= max_leaders <= 64: one is free
            q.lanes_taken |= (uint64_t)1 << lane;
            while (!q.pending.empty() && !me.done) {
                // another batch is in flight: a short wait lets the callers it is about to release come back with their
                // next request — larger batches, fewer invocations
                if (gathers && q.leaders > 1 && q.pending.size() < q.gather_min) {
                    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(q.gather_us);
                    while (q.pending.size() < q.gather_min && !me.done && q.cv.wait_until(lk, until) != std::cv_status::timeout) {
                    }
                    if (me.done) break;
                    if (q.pending.empty()) continue;
                }
                batch.clear();
                const Req* front = q.pending.front();
                for (auto it = q.pending.begin(); it != q.pending.end() && batch.size() < q.batch_max;) {
                    if (same(*front, **it)) {
                        batch.push_back(*it);
                        it = q.pending.erase(it);
                    } else {
                        ++it;
                    }
                }
                lk.unlock();
                run(batch, lane);
                lk.lock();
                for (Req* r : batch) r->done = true;
                q.cv.notify_all();
            }
            q.lanes_taken &= ~((uint64_t)1 << lane);
            --q.leaders;
            q.cv.notify_all();  // whoever still waits leads what is left
        } else if (!idled) {
            idled = true;
            lk.unlock();
            me.side_work();
            lk.lock();
        } else {
            q.cv.wait(lk);
        }
    }
    lk.unlock();
    me.side_work();
}

// How a SlotPool grows.  Chunked: as callers need slots, 4, 4, 8, 16, 16, ... at a time — a handle that one thread uses
// at a time holds four slots, sixteen concurrent callers grow the pool to what they use.  AllAtOnce: max_slots with the
// first caller.
enum class SlotGrowth { Chunked, AllAtOnce };

// Up to max_slots staging slots of slot_bytes each, carved out of chunks that Alloc supplies: `void* alloc(size_t)`
// (NULL on failure) and `void free(void*)`.  A mutex of its own: callers take and return slots beside the queue.
template <class Alloc>
class SlotPool {
  public:
    SlotPool(size_t slot_bytes, int max_slots, SlotGrowth growth, Alloc alloc = Alloc())
        : slot_bytes_(slot_bytes), max_slots_(max_slots), growth_(growth), alloc_(alloc) {
        free_.reserve((size_t)max_slots);  // acquire and release never allocate host memory of their own
        chunks_.reserve((size_t)max_slots);
    }
    ~SlotPool() {
        for (void* c : chunks_) alloc_.free(c);
    }
    SlotPool(const SlotPool&) = delete;
    SlotPool& operator=(const SlotPool&) = delete;

    // NULL when every slot is taken and the pool cannot grow: the caller does without one
    unsigned char* acquire() {
        std::lock_guard<std::mutex> lk(mu_);
        if (free_.empty() && !failed_ && allocated_ < max_slots_) {
            int grow = growth_ == SlotGrowth::AllAtOnce ? max_slots_ : allocated_ < 8 ? 4 : allocated_ < 16 ? 8 : 16;
            if (grow > max_slots_ - allocated_) grow = max_slots_ - allocated_;
            unsigned char* chunk = (unsigned char*)alloc_.alloc((size_t)grow * slot_bytes_);
            if (!chunk) {
                failed_ = true;  // not tried again
            } else {
                chunks_.push_back(chunk);
                allocated_ += grow;
                for (int i = grow; i-- > 0;) free_.push_back(chunk + (size_t)i * slot_bytes_);
            }
        }
        if (free_.empty()) return nullptr;
        unsigned char* p = free_.back();
        free_.pop_back();
        return p;
    }
    void release(unsigned char* p) {
        if (!p) return;
        std::lock_guard<std::mutex> lk(mu_);
        free_.push_back(p);
    }

  private:
    const size_t slot_bytes_;
    const int max_slots_;
    const SlotGrowth growth_;
    Alloc alloc_;
    std::mutex mu_;
    std::vector<void*> chunks_;
    std::vector<unsigned char*> free_;
    int allocated_ = 0;
    bool failed_ = false;
};

}  // namespace kzgamd
