// The side lane of calm_gemm: host bookkeeping (no device code).
// Weight gradients are leaf gradients: nothing reads them before the end of the backward.  A caller may therefore issue
// a weight-gradient GEMM on a second, lowest-priority stream the library owns (one per device) so that it fills the CUs
// while the caller's stream runs kernels that leave the matrix pipe idle:
//     fork(main)            an event recorded on `main`, the lane waits for it: the lane sees the operands finished
//     launch_stream(main)   the stream a lane launch goes to (counts the launch)
//     join(main)            an event recorded on the lane, `main` waits for it; nothing if no launch since the last join
// While `main` is capturing, or the lane is switched off, fork does nothing and launch_stream returns `main`: a captured
// graph keeps the shape it has without the lane.
// The runtime calls come through `Rt` (gemm.hip: the HIP runtime; tests/host/lane_book_main.cpp: a recording stub), so
// that this file can be compiled and run on its own under a host sanitizer.
#pragma once
#include <stdint.h>
#include <mutex>

namespace calm_lane {

constexpr int RING = 8;          // events per device, used round robin (a wait takes the record that precedes it, so
                                 // re-recording an event that an earlier wait named does not disturb that wait)
constexpr int MAX_DEVICES = 16;

struct Stats {                   // calm_gemm_lane_stats
    int64_t forks = 0;           // forks that recorded an event
    int64_t launches = 0;        // launches that went to a lane
    int64_t joins = 0;           // joins that recorded an event
    int64_t events = 0;          // events recorded (forks + joins)
};

template <class Rt>
class Book {
    using Stream = typename Rt::Stream;
    using Event = typename Rt::Event;
    struct Lane {
        Stream s{};
        Event ev[RING]{};
        unsigned next = 0;
        bool ready = false;
        long pending = 0;        // launches since the last join
    };
    Lane lanes_[MAX_DEVICES];
    Stats stats_;
    std::mutex mu_;

    // the lane of the current device, created at first use; nullptr with rc set on failure
    Lane* lane(bool create, int& rc) {
        int dev = 0;
        rc = Rt::device(&dev);
        if (rc) return nullptr;
        if (dev < 0 || dev >= MAX_DEVICES) { rc = -3; return nullptr; }      // CALM_E_UNSUPP
        Lane& l = lanes_[dev];
        if (l.ready || !create) return &l;
        Stream s{};
        rc = Rt::stream_create(&s);
        if (rc) return nullptr;
        for (int i = 0; i < RING; ++i) {
            rc = Rt::event_create(&l.ev[i]);
            if (rc) return nullptr;      // (what was created stays allocated: a failure here ends the job)
        }
        l.s = s;
        l.ready = true;
        return &l;
    }

    // record the next event of the ring on `from`, make `to` wait for it
    int hand_over(Lane& l, Stream from, Stream to) {
        Event e = l.ev[l.next++ % RING];
        int rc = Rt::record(e, from);
        if (rc) return rc;
        ++stats_.events;
        return Rt::wait(to, e);
    }

public:
    // `on`: CALM_GEMM_OPT_LANE.  0, or the runtime's error.
    int fork(bool on, Stream main) {
        if (!on) return 0;
        bool cap = false;
        int rc = Rt::capturing(main, &cap);
        if (rc || cap) return rc;
        std::lock_guard<std::mutex> g(mu_);
        Lane* l = lane(true, rc);
        if (!l) return rc;
        rc = hand_over(*l, main, l->s);
        if (!rc) ++stats_.forks;
        return rc;
    }

    // *out: the stream of a lane launch made now.
    int launch_stream(bool on, Stream main, Stream* out) {
        *out = main;
        if (!on) return 0;
        bool cap = false;
        int rc = Rt::capturing(main, &cap);
        if (rc || cap) return rc;
        std::lock_guard<std::mutex> g(mu_);
        Lane* l = lane(true, rc);
        if (!l) return rc;
        ++l->pending;
        ++stats_.launches;
        *out = l->s;
        return 0;
    }

    // Joins whatever went to the lane, whether or not the option is still on.
    int join(Stream main) {
        std::lock_guard<std::mutex> g(mu_);
        bool any = false;
        for (const Lane& l : lanes_) any = any || l.pending > 0;
        if (!any) return 0;                                   // (no runtime call: valid without a device)
        int rc = 0;
        Lane* l = lane(false, rc);
        if (!l || l->pending == 0) return rc;
        bool cap = false;
        rc = Rt::capturing(main, &cap);
        if (rc || cap) return rc;                             // (lane launches never start inside a capture)
        rc = hand_over(*l, l->s, main);
        if (rc) return rc;
        l->pending = 0;
        ++stats_.joins;
        return 0;
    }

    Stats stats() {
        std::lock_guard<std::mutex> g(mu_);
        return stats_;
    }
};

}  // namespace calm_lane
