// Stand-alone host program around the bookkeeping of calm_gemm's side lane (calm-vit-dte_amd/csrc/gemm_lane.h): the event
// ring and the fork / launch / join counters, with a runtime that records what it is asked to do instead of doing it.
// No device, no HIP.  Build and run (tests/test_wgrad_lane_cpu.py does, without the sanitizers):
//     c++ -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -I calm-vit-dte_amd/csrc
//         tests/host/lane_book_main.cpp -o lane_book && ./lane_book          (or -fsanitize=thread)
// Exit status 0 and "lane_book: ok" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <thread>
#include <vector>

#include "gemm_lane.h"

namespace {

struct Call { char what; int stream; int event; };      // 'r' record(event, stream), 'w' wait(stream, event)
std::vector<Call> g_calls;
std::vector<std::unique_ptr<int>> g_event_cells;      // the stub owns its events (the library never destroys a lane)
int g_streams = 0, g_events = 0, g_device = 0, g_capturing_stream = -1, g_fail_event_at = -1;

struct StubRt {
    using Stream = int;          // 0: unset; main streams are 100.., lanes 1..
    using Event = int*;          // heap cells: a sanitizer sees every use of an event that was never created
    static int device(int* d) { *d = g_device; return 0; }
    static int capturing(Stream s, bool* c) { *c = s == g_capturing_stream; return 0; }
    static int stream_create(Stream* s) { *s = ++g_streams; return 0; }
    static int event_create(Event* e) {
        if (g_events == g_fail_event_at) return 7;
        g_event_cells.emplace_back(new int(g_events++));
        *e = g_event_cells.back().get();
        return 0;
    }
    static int record(Event e, Stream s) { g_calls.push_back({'r', s, *e}); return 0; }
    static int wait(Stream s, Event e) { g_calls.push_back({'w', s, *e}); return 0; }
};

int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

using Book = calm_lane::Book<StubRt>;

}  // namespace

int main() {
    const int MAIN = 100;
    {   // nothing to do: no runtime call, no lane, no event
        Book b;
        int s = -1;
        CHECK(b.fork(false, MAIN) == 0);
        CHECK(b.launch_stream(false, MAIN, &s) == 0 && s == MAIN);
        CHECK(b.join(MAIN) == 0);
        CHECK(g_calls.empty() && g_streams == 0 && g_events == 0);
        const calm_lane::Stats st = b.stats();
        CHECK(st.forks == 0 && st.launches == 0 && st.joins == 0 && st.events == 0);
    }
    {   // fork without a launch: the join issues nothing; with launches: one record on the lane, one wait on main
        Book b;
        CHECK(b.fork(true, MAIN) == 0);
        CHECK(g_streams == 1 && g_events == calm_lane::RING);
        CHECK(g_calls.size() == 2 && g_calls[0].what == 'r' && g_calls[0].stream == MAIN && g_calls[1].what == 'w' &&
              g_calls[1].stream == 1 && g_calls[0].event == g_calls[1].event);
        CHECK(b.join(MAIN) == 0);
        CHECK(g_calls.size() == 2 && b.stats().joins == 0);
        int s = -1;
        for (int i = 0; i < 3; ++i) {
            CHECK(b.fork(true, MAIN) == 0);
            CHECK(b.launch_stream(true, MAIN, &s) == 0 && s == 1);
        }
        const size_t n = g_calls.size();
        CHECK(n == 2 + 3 * 2);
        CHECK(b.join(MAIN) == 0);
        CHECK(g_calls.size() == n + 2 && g_calls[n].what == 'r' && g_calls[n].stream == 1 && g_calls[n + 1].what == 'w' &&
              g_calls[n + 1].stream == MAIN && g_calls[n].event == g_calls[n + 1].event);
        CHECK(b.join(MAIN) == 0);                        // joined: nothing more
        CHECK(g_calls.size() == n + 2);
        calm_lane::Stats st = b.stats();
        CHECK(st.forks == 4 && st.launches == 3 && st.joins == 1 && st.events == 5);
        // the ring: RING consecutive hand-overs use RING different events, then the first again
        g_calls.clear();
        for (int i = 0; i < calm_lane::RING + 1; ++i) CHECK(b.fork(true, MAIN) == 0);
        for (int i = 0; i < calm_lane::RING; ++i)
            for (int j = 0; j < i; ++j) CHECK(g_calls[2 * i].event != g_calls[2 * j].event);
        CHECK(g_calls[2 * calm_lane::RING].event == g_calls[0].event);
        CHECK(g_streams == 1 && g_events == calm_lane::RING);   // one lane, one ring: created once
        // a launch left on the lane is joined even after the option went off
        CHECK(b.launch_stream(true, MAIN, &s) == 0 && s == 1);
        g_calls.clear();
        CHECK(b.fork(false, MAIN) == 0 && b.launch_stream(false, MAIN, &s) == 0 && s == MAIN && g_calls.empty());
        CHECK(b.join(MAIN) == 0 && g_calls.size() == 2 && b.stats().joins == 2);
    }
    {   // a capturing main stream: fork does nothing, the launch stays on it; a lane launch made before is not joined
        // into the capture
        Book b;
        int s = -1;
        g_calls.clear();
        g_capturing_stream = 200;
        CHECK(b.fork(true, 200) == 0 && b.launch_stream(true, 200, &s) == 0 && s == 200 && b.join(200) == 0);
        CHECK(g_calls.empty() && b.stats().launches == 0);
        CHECK(b.fork(true, MAIN) == 0 && b.launch_stream(true, MAIN, &s) == 0 && s != MAIN);
        const size_t n = g_calls.size();
        CHECK(b.join(200) == 0 && g_calls.size() == n);
        CHECK(b.join(MAIN) == 0 && g_calls.size() == n + 2);
        g_capturing_stream = -1;
    }
    {   // one lane per device; a join only joins the current device's lane
        Book b;
        int s0 = -1, s1 = -1;
        g_device = 0;
        CHECK(b.launch_stream(true, MAIN, &s0) == 0);
        g_device = 1;
        CHECK(b.launch_stream(true, MAIN + 1, &s1) == 0 && s1 != s0);
        g_calls.clear();
        CHECK(b.join(MAIN + 1) == 0 && g_calls.size() == 2 && g_calls[0].stream == s1);
        CHECK(b.join(MAIN + 1) == 0 && g_calls.size() == 2);
        g_device = 0;
        CHECK(b.join(MAIN) == 0 && g_calls.size() == 4 && g_calls[2].stream == s0);
        g_device = calm_lane::MAX_DEVICES;               // beyond the table: an error, no write
        CHECK(b.fork(true, MAIN) != 0);
        g_device = 0;
    }
    {   // a runtime failure while the ring is created is returned, and no launch is routed to a half-made lane
        Book b;
        int s = -1;
        g_fail_event_at = g_events + 3;
        CHECK(b.fork(true, MAIN) == 7);
        CHECK(b.launch_stream(true, MAIN, &s) == 7 && s == MAIN);
        g_fail_event_at = -1;
    }
    {   // calls from two threads (the autograd engine's device thread and the caller's): counters stay consistent
        Book b;
        g_calls.reserve(1 << 16);
        auto work = [&b](int main_stream) {
            int s = -1;
            for (int i = 0; i < 200; ++i) {
                if (b.fork(true, main_stream) || b.launch_stream(true, main_stream, &s)) abort();
                if (i % 10 == 9 && b.join(main_stream)) abort();
            }
        };
        std::thread t1(work, MAIN), t2(work, MAIN + 1);
        t1.join();
        t2.join();
        CHECK(b.join(MAIN) == 0);
        const calm_lane::Stats st = b.stats();
        CHECK(st.forks == 400 && st.launches == 400 && st.events == st.forks + st.joins && st.joins >= 20);
    }
    if (g_failed) return 1;
    printf("lane_book: ok\n");
    return 0;
}
