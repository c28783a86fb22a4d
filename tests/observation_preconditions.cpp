// The host-side bookkeeping of adjoint observations (trm_host.hpp) on contexts built by hand: no GPU call.  An observation on the
// checkpointed tape closes the open segment, so that the next taped step opens one and takes a slot; what an observation holds on the
// device is its arrays and its level list, laid out in one allocation.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_host.hpp"
#include <cassert>

namespace trmh {
int fail(trm_ctx*, int code, const std::string&) { return code; }
}  // namespace trmh
using namespace trmh;

int main() {
    // K = 4 steps to a slot; the run of the tests: 3 steps, an observation, 2 steps, an observation, 1 step
    trm_ctx t;
    t.ckpt_interval = 4;
    t.tape_cap = 3;
    const double dt = 300.0;
    assert(open_segment_room(&t, dt) == 0 && tape_slots_needed(&t, dt, 3) == 1);
    tape_append(&t, dt, 3);
    assert(taped_steps(&t) == 3 && tape_slots_used(&t) == 1 && open_segment_room(&t, dt) == 1);
    assert(tape_slots_needed(&t, dt, 1) == 0 && tape_slots_needed(&t, dt, 2) == 1);
    t.tape_seg_closed = true;                                   // (what a registration at position 3 does)
    assert(open_segment_room(&t, dt) == 0 && tape_slots_needed(&t, dt, 0) == 0);
    assert(tape_slots_needed(&t, dt, 1) == 1 && tape_slots_needed(&t, dt, 2) == 1 && tape_slots_needed(&t, dt, 5) == 2);
    tape_append(&t, dt, 0);                                     // (no step: the segment stays closed)
    assert(t.tape_seg_closed && tape_slots_used(&t) == 1);
    tape_append(&t, dt, 2);
    assert(!t.tape_seg_closed && taped_steps(&t) == 5 && tape_slots_used(&t) == 2);
    assert(t.tape_segs[0].first == 0 && t.tape_segs[0].len == 3 && t.tape_segs[1].first == 3 && t.tape_segs[1].len == 2 && t.tape_segs[1].slot == 1);
    assert(open_segment_room(&t, dt) == 2);
    t.tape_seg_closed = true;                                   // (position 5)
    assert(tape_slots_needed(&t, dt, 1) == 1 && tape_slots_needed(&t, dt, 1) <= t.tape_cap - tape_slots_used(&t));
    tape_append(&t, dt, 1);
    assert(taped_steps(&t) == 6 && tape_slots_used(&t) == 3 && t.tape_segs[2].first == 5 && t.tape_segs[2].len == 1 && !t.tape_seg_closed);
    t.tape_seg_closed = true;                                   // (position 6 = n: the tape is full)
    assert(tape_slots_needed(&t, dt, 1) == 1 && tape_slots_needed(&t, dt, 1) > t.tape_cap - tape_slots_used(&t));
    // a segment that is full, or a call under another dt, opens a segment with or without an observation: the same count
    trm_ctx u;
    u.ckpt_interval = 4;
    tape_append(&u, dt, 4);
    const long long open_full = tape_slots_needed(&u, dt, 3), open_other_dt = tape_slots_needed(&u, 0.5 * dt, 3);
    u.tape_seg_closed = true;
    assert(tape_slots_needed(&u, dt, 3) == open_full && open_full == 1 && tape_slots_needed(&u, 0.5 * dt, 3) == open_other_dt);
    // the per-step tape has no segments: nothing to close
    trm_ctx s;
    s.tape_seg_closed = true;
    assert(tape_slots_needed(&s, dt, 7) == 7);
    tape_append(&s, dt, 7);
    assert(taped_steps(&s) == 7 && s.tape_segs.empty());
    // what an observation holds: `arrays` arrays of [nlevels][Nh] doubles, then nlevels int32
    const long Nh = 5;
    std::vector<double> block(2 * 3 * Nh + 2);                  // (room for 3 int32 behind the doubles)
    trm_ctx::Observation o{3, trm_ctx::OBSERVE_MISFIT, 3, 2, block.data()};
    assert(o.array(0, Nh) == block.data() && o.array(1, Nh) == block.data() + 3 * Nh && o.array(2, Nh) == nullptr);
    assert((const void*)o.levels(Nh) == (const void*)(block.data() + 2 * 3 * Nh));
    assert(o.bytes(Nh) == 2 * 3 * Nh * 8 + 3 * 4 && (size_t)o.bytes(Nh) <= block.size() * sizeof(double));
    trm_ctx::Observation lin{0, TRM_ADJOINT_TEMPERATURE, 1, 1, block.data()};
    assert(lin.array(1, Nh) == nullptr && lin.bytes(Nh) == Nh * 8 + 4 && (const void*)lin.levels(Nh) == (const void*)(block.data() + Nh));
    return 0;
}
