// stage_selftest -- host-side bookkeeping of the library, driven on the CPU (no device, no HIP call is reached):
//   1. HostStage::take() beyond the pinned block -> nullptr, and the call's wait() answers VIS_E_NOMEM instead of copying past the block
//   2. vis_ensure_pin() asked to grow (= free + re-allocate) the block while a HostStage is alive -> VIS_E_STATE, block untouched
//   3. ReaderGuard (the batch path's buffer sets): which reader events a writer would wait for, and align_reader(): which alignment a
//      write of caller memory waits for; StreamScope, the alignments' ring and note_readers(): the bookkeeping of on_pose_stream()
//   4. Carver / the one buffer list of a host-pointer call (vis_carve): the measuring and the binding pass walk the same offsets, a take
//      beyond the block is refused, and the pinned bound derived from the list holds a stage that passes every buffer up and down
//   5. vis_carve_block / vis_grow_block (the context's grow-only device-rows workspaces) on host buffers that stand in for blocks: a list fits a
//      block of exactly its measured size, a block that is large enough is neither touched nor reported as replaced, a list of nothing asks for
//      nothing.  The growing branch itself (drain, free, allocate) needs a device: tests/test_block_growth_gpu.py drives it
//   6. Turn (which of a plan's two carried rows a follow-up launch continues): the table of repeated, skipped, forgotten and seeded runs
// (round 5's host SIGSEGV, gpurun_out/r5r_gdb.log: a stage that kept the address of a block a later vis_ensure_pin had freed; see
// csrc/vis_internal.h at HostStage).  Compiled by `make -C vi-slam_amd/csrc selftest` with hipcc as host code against the library;
// tests/test_abi.py runs it.  Prints one line per check and exits non-zero on the first failure.
#include "../csrc/vis_internal.h"
#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(cond) do { const bool ok_ = (cond); std::printf("%s  %s\n", ok_ ? "ok  " : "FAIL", #cond); if (!ok_) fails++; } while (0)

int main() {
    vis_ctx c;                                         // (default members only: no stream, no device)
    std::vector<char> block(1024);
    c.h_pin = block.data(); c.h_pin_bytes = block.size(); c.h_pin_dev = nullptr;
    {
        HostStage hs(&c);
        CHECK(c.stage_live == 1);
        void* a = hs.take(512);
        CHECK(a == block.data());
        void* b = hs.take(500);                        // 512 + 500 fits (offsets are 64-byte aligned: 512 is)
        CHECK(b == block.data() + 512);
        void* d = hs.take(64);                         // 1012 -> 1024 aligned + 64 > 1024
        CHECK(d == nullptr && hs.overflow);
        const unsigned long long waits = c.n_host_waits;
        CHECK(hs.wait() == VIS_E_NOMEM && c.n_host_waits == waits);      // refused before any device call
        // a block that must grow while the stage lives: refused, nothing freed, nothing allocated
        CHECK(vis_ensure_pin(&c, 4096) == VIS_E_STATE && c.h_pin == block.data() && c.h_pin_bytes == block.size());
        CHECK(vis_ensure_pin(&c, 1000) == VIS_OK);     // large enough already: no replacement, allowed under a live stage
    }
    CHECK(c.stage_live == 0);
    {
        vis_ctx e;                                     // no block at all
        HostStage hs(&e);
        CHECK(hs.take(4) == nullptr && hs.overflow && hs.wait() == VIS_E_NOMEM);
        char src[8] = {0};
        hs.up((void*)0x1000, src, 8);                  // an upload on an overflowing stage copies nothing and queues nothing
        CHECK(hs.up_n == 0 && e.n_copies == 0);
    }
    c.h_pin = nullptr; c.h_pin_bytes = 0;              // (the vector owns the memory)
    {
        // stand-in handles: only compared, never passed to the runtime
        const hipStream_t sM = (hipStream_t)0x10, sP = (hipStream_t)0x20;
        const hipEvent_t e1 = (hipEvent_t)0x100, e2 = (hipEvent_t)0x200, e3 = (hipEvent_t)0x300;
        ReaderGuard g;
        CHECK(!g.stream[0] && !g.event[0]);                                   // nothing to wait for
        g.note(sP, e1); g.note(sP, e2);                                       // a later reader on the same stream stands for the earlier one
        CHECK(g.stream[0] == sP && g.event[0] == e2 && !g.stream[1]);
        g.note(sM, e3);                                                       // readers on two streams: both waited for
        CHECK(g.stream[0] == sP && g.event[0] == e2 && g.stream[1] == sM && g.event[1] == e3 && !g.stream[2]);
        g.note(sP, e1);                                                       // (each stream keeps its own slot)
        CHECK(g.event[0] == e1 && g.event[1] == e3 && !g.stream[2]);
        g.clear();
        CHECK(!g.stream[0] && !g.event[0] && !g.stream[1] && !g.event[1]);
        // caller memory and the alignments on the pose stream
        vis_ctx a;
        uint8_t frames[5][64];                                                // (frames 0-3; frames[4] = one past frame 3)
        CHECK(align_reader(&a, nullptr, nullptr) == nullptr);                 // no alignment at all
        CHECK(align_reader(&a, frames[0], frames[1]) == nullptr);
        a.align[1] = {e1, frames[0], frames[2]}; a.align_last = 1;           // one alignment, of frames 0-1
        CHECK(align_reader(&a, frames[1], frames[2]) == e1);                  // a range it read
        CHECK(align_reader(&a, frames[2], frames[4]) == nullptr);             // a range it did not read, no older alignment
        CHECK(align_reader(&a, nullptr, nullptr) == e1);                      // range not known: the latest
        a.align[0] = {e2, frames[2], frames[4]}; a.align_last = 0;           // a later one, of frames 2-3
        CHECK(align_reader(&a, frames[3], frames[4]) == e2);                  // a range the last alignment read
        CHECK(align_reader(&a, frames[0], frames[1]) == e1);                  // one it did not read while an older one is pending
        CHECK(align_reader(&a, frames[1], frames[3]) == e2);                  // overlapping both: the latest stands for the older
        CHECK(align_reader(&a, nullptr, nullptr) == e2);
        // the stream switch of the batch path: restored when the block is left by an early return, nested scopes in order
        const hipStream_t sA = (hipStream_t)0x30;
        vis_ctx f;
        f.stream = sA;
        const int rc = [&]() -> int { StreamScope on(&f, sP); if (f.stream == sP) return VIS_E_HIP; return VIS_OK; }();
        CHECK(rc == VIS_E_HIP && f.stream == sA);
        {
            StreamScope onM(&f, sM);
            { StreamScope onP(&f, sP); CHECK(f.stream == sP); }
            CHECK(f.stream == sM);
        }
        CHECK(f.stream == sA);
        // the alignments' ring: two slots in turn; nothing changes before the commit
        f.ev_align_done[0] = e1; f.ev_align_done[1] = e2;
        CHECK(align_ring_next(&f) == e2 && align_ring_next(&f) == e2);          // "next" alone commits nothing
        CHECK(f.align_last == 0 && align_reader(&f, nullptr, nullptr) == nullptr);
        align_ring_commit(&f, frames[0], frames[2]);                          // frames 0-1
        CHECK(f.align_last == 1 && align_reader(&f, frames[1], frames[2]) == e2 && align_reader(&f, frames[2], frames[4]) == nullptr);
        CHECK(align_ring_next(&f) == e1);
        align_ring_commit(&f, frames[2], frames[4]);                          // frames 2-3: the other slot
        CHECK(f.align_last == 0 && align_ring_next(&f) == e2);
        CHECK(align_reader(&f, frames[3], frames[4]) == e1);                  // overlapping the new one: the new event
        CHECK(align_reader(&f, frames[0], frames[1]) == e2);                  // disjoint: the older one
        // a guard list with a null entry: the event is noted on the others only
        ReaderGuard g1, g2;
        note_readers({&g1, nullptr, &g2}, sP, e3);
        CHECK(g1.stream[0] == sP && g1.event[0] == e3 && !g1.stream[1] && g2.stream[0] == sP && g2.event[0] == e3 && !g2.stream[1]);
    }
    {
        // one buffer list, as an entry point writes it (odd sizes: every take pays its alignment); d[2] goes up and comes down
        const size_t sizes[4] = {1000, 7, 300, 4097};
        void* d[4];
        auto layout = [&](Carver& cv) { for (int i = 0; i < 4; i++) d[i] = cv.take<char>(sizes[i]); };
        Carver measure{nullptr, 0, SIZE_MAX};
        layout(measure);
        CHECK(!measure.overflow && measure.n == 4 && !d[0] && !d[3]);          // measuring hands out no address
        CHECK(measure.off == 1792 + 4097);                                    // 0, 1024, 1280, 1792: 256-byte aligned offsets
        std::vector<char> dev(measure.off + 1);
        Carver bound{dev.data(), 0, measure.off};                             // bound at exactly the measured size
        layout(bound);
        CHECK(!bound.overflow && bound.off == measure.off);                   // the measured size is what a bound pass consumes
        CHECK(d[0] == dev.data() && d[1] == dev.data() + 1024 && d[2] == dev.data() + 1280 && d[3] == dev.data() + 1792);   // identical offsets
        Carver tight{dev.data(), 0, measure.off - 1};                         // one byte short: the last take ends beyond the block
        layout(tight);
        CHECK(tight.overflow && d[2] == dev.data() + 1280 && d[3] == nullptr && tight.off == 1280 + 300);
        CHECK(tight.take<char>(1) == nullptr && tight.off == 1280 + 300);     // nothing is handed out after an overflow
        // the pinned bound of the list, two ways: a stage that uploads and downloads every buffer once fits
        std::vector<char> pin(measure.pin_bound(2)), src(4097);
        vis_ctx p;
        p.h_pin = pin.data(); p.h_pin_bytes = pin.size(); p.h_pin_dev = nullptr;
        {
            HostStage hs(&p);
            for (int i = 0; i < 4; i++) CHECK(hs.take(sizes[i]) != nullptr);                              // (up(): take + memcpy + a queued copy)
            for (int i = 0; i < 4; i++) CHECK(hs.take(std::max(sizes[i], (size_t)4)) != nullptr);         // (down(): take + a queued copy)
            CHECK(!hs.overflow && hs.off <= pin.size());
        }
        p.h_pin = nullptr; p.h_pin_bytes = 0;
        // the same list carved into a grow-only block of the context (vis_carve_block), host buffers standing in for device blocks
        vis_ctx q;
        DevBlock exact{dev.data(), measure.off};                              // exactly the measured size: fits, so the grow rule changes nothing
        bool replaced = true;
        CHECK(vis_carve_block(&q, exact, "selftest", layout, 0, &replaced) == VIS_OK && !replaced);
        CHECK(exact.p == dev.data() && exact.bytes == measure.off);           // the measured size is what the bound pass consumes: no overflow
        CHECK(d[0] == dev.data() && d[1] == dev.data() + 1024 && d[2] == dev.data() + 1280 && d[3] == dev.data() + 1792);
        std::vector<char> big(3 * measure.off);
        DevBlock roomy{big.data(), big.size()};                               // larger than the list, and than the list's floor: neither touched nor replaced
        replaced = true;
        CHECK(vis_carve_block(&q, roomy, "selftest", layout, 2 * measure.off, &replaced) == VIS_OK && !replaced);
        CHECK(roomy.p == big.data() && roomy.bytes == big.size() && d[0] == big.data() && d[3] == big.data() + 1792);
        DevBlock none;                                                        // a list of nothing asks for nothing: no block, no allocation
        void* z = dev.data();
        replaced = true;
        CHECK(vis_carve_block(&q, none, "selftest", [&](Carver& cv) { z = cv.take<char>(0); }, 0, &replaced) == VIS_OK && !replaced);
        CHECK(none.p == nullptr && none.bytes == 0 && z == nullptr);
        CHECK(vis_grow_block(&q, none, 0, "selftest", &replaced) == VIS_OK && !replaced && none.p == nullptr);
        CHECK(vis_grow_block(&q, exact, measure.off, "selftest") == VIS_OK && exact.p == dev.data());
        CHECK(q.err.empty());
    }
    {
        // the turn of a plan's two carried rows (Turn): the table of cases; a pick is committed unless it says otherwise
        Turn t;
        auto is = [](Turn::Pick p, int slot, bool have) { return p.slot == slot && p.have == have; };
        auto step = [&](int run) { const Turn::Pick p = t.pick(run); t.commit(p, run); return p; };
        CHECK(t.in == 0 && t.run == -1 && !t.have);
        CHECK(is(step(0), 1, false));                                         // 1  fresh: nothing to read, the launch writes row 0
        CHECK(is(step(0), 1, false));                                         // 2  repeated for the same run: the same answer
        CHECK(is(step(1), 0, true));                                          // 3  the next run reads row 0 and writes row 1
        CHECK(is(step(1), 0, true));                                          // 4  repeated: reads row 0 again
        CHECK(is(step(3), 1, false));                                         // 5  run 2 was skipped: nothing to read
        const Turn before = t;
        CHECK(is(t.pick(4), 0, true) && t.in == before.in && t.run == before.run && t.have == before.have);   // 6  a pick alone changes nothing
        t.forget();
        CHECK(t.in == before.in && is(step(4), 0, false));                    // 7  forgotten: nothing to read; `in` survived
        CHECK(t.seed_slot() == 1);                                            // 8  a record seeded at run 4 goes where a call for run 4 would have written
        t.seeded(4);
        CHECK(!t.have && is(step(5), 1, true));                               //    and run 5 reads it
        const int seed = t.seed_slot();
        t.seeded(5); t.forget();
        CHECK(seed == 0 && is(step(5), 0, false));                            // 9  forgotten after a seed: nothing to read
        Turn u;                                                               // 10 fresh, seeded at run 0
        CHECK(u.seed_slot() == 1);
        u.seeded(0);
        CHECK(is(u.pick(1), 1, true));                                        //    run 1 reads the seed
        CHECK(is(u.pick(0), 0, false));                                       //    a call for the seeded run itself writes row 1: it overwrites the seed (pinned as it is)
        u.commit(u.pick(1), 1);
        CHECK(is(u.pick(0), 0, false));                                       //    (and so after run 1 was committed)
    }
    std::printf(fails ? "stage_selftest FAILED (%d)\n" : "stage_selftest passed\n", fails);
    return fails ? 1 : 0;
}
