// Exercises the host-side preconditions of the derivative launches (trm_launch_derivative.inl) on contexts built by hand: no GPU call.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_launch_derivative.inl"
#include <cassert>

namespace trmh {
static std::string last;
int fail(trm_ctx*, int code, const std::string& msg) { last = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

int main() {
    trm_ctx c;
    c.Nh = 3; c.Nz = 4; c.Nzp = 4;
    c.tape_cap = 8;
    // tape range: the per-step tape and a segment
    assert(tape_range_ok(&c, 8, 0, "r") == TRM_OK && tape_range_ok(&c, 8, 1, "r") == TRM_EINVAL && tape_range_ok(&c, -1, 0, "r") == TRM_EINVAL);
    assert(segment_range_ok(&c, TRM_ADJOINT_MAX_INTERVAL, 7, "s") == TRM_OK && segment_range_ok(&c, TRM_ADJOINT_MAX_INTERVAL + 1, 7, "s") == TRM_EINVAL);
    assert(segment_range_ok(&c, 1, 8, "s") == TRM_EINVAL && last == "s: the launch leaves the tape");
    // store count of the strided record
    int slot = 6;
    assert(strided_stores_ok(&c, 9, slot, 1, 4, "k") == TRM_OK && slot == 6);          // stores before steps 1 and 5: slots 6, 7
    assert(strided_stores_ok(&c, 10, slot, 1, 4, "k") == TRM_EINVAL);                   // ... and 9: slot 8 is outside
    slot = 8;                                                                        // (a full tape)
    assert(strided_stores_ok(&c, 3, slot, 3, 4, "k") == TRM_OK && slot == 0);          // no store: any slot inside the tape
    assert(strided_stores_ok(&c, 3, slot, 0, 0, "k") == TRM_EINVAL && last == "k: bad launch");
    // missing accumulators
    double x[4] = {};
    assert(gradients_ok<RIDE_NONE>(&c, 1, "g") == TRM_OK);
    assert(gradients_ok<RIDE_BC>(&c, 1, "g") == TRM_EINVAL && last == "g: no accumulators");
    for (int q = 0; q < 3; ++q) c.d_adj_bc[q] = x;
    assert(gradients_ok<RIDE_BC>(&c, 1, "g") == TRM_EINVAL);
    c.d_adj_bc[3] = x;
    assert(gradients_ok<RIDE_BC>(&c, 1, "g") == TRM_OK);
    assert(gradients_ok<RIDE_PARAM>(&c, 1, "g") == TRM_EINVAL && last == "g: no accumulators");
    for (auto& q : c.d_adj_param) q = x;
    assert(gradients_ok<RIDE_PARAM>(&c, 1, "g") == TRM_OK);
    // series: rows, and a node accumulator of the shape of every series
    assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_EINVAL && last == "g: no series rows, or the generic boundary kinds");
    c.d_series_table = x;
    assert(series_rows_ok(&c, 0, "g") == TRM_OK && series_rows_ok(&c, 1, "g") == TRM_EINVAL);
    c.d_series_rows = x;
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
    trm_ctx::Series sr;
    sr.is_bc = true; sr.var = TRM_BCV_TEMPERATURE; sr.side = TRM_TOP; sr.cap = 5;
    c.series.push_back(sr);
    assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_EINVAL && last == "g: a series without an accumulator of its shape");
    c.d_adj_bcs[SLOT_T_TOP] = x;
    c.adj_bcs_nt[SLOT_T_TOP] = 4;
    assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_EINVAL);
    c.adj_bcs_nt[SLOT_T_TOP] = 5;
    assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_OK);
    assert(series_nodes_ok(&c, c.d_tan_bcs, c.tan_bcs_nt, "t", "seeds") == TRM_EINVAL && last == "t: a series without seeds of its shape");
    // the tape's bookkeeping (trm_host.hpp): checkpointed, K = 4 steps to a slot, 3 slots
    trm_ctx t;
    t.ckpt_interval = 4;
    t.tape_cap = 3;
    auto seg = [&](size_t s, int first, int len, double dt, int slot) {
        const trm_ctx::TapeSegment& g = t.tape_segs[s];
        return g.first == first && g.len == len && g.dt == dt && g.slot == slot;
    };
    assert(taped_steps(&t) == 0 && open_segment_room(&t, 1.0) == 0 && tape_slots_used(&t) == 0);                  // an empty tape
    assert(tape_slots_needed(&t, 1.0, 0) == 0 && tape_slots_needed(&t, 1.0, 1) == 1 && tape_slots_needed(&t, 1.0, 4) == 1 && tape_slots_needed(&t, 1.0, 5) == 2);
    assert(tape_slots_needed(&t, 1.0, 12) == 3 && tape_slots_needed(&t, 1.0, 13) == 4);                            // exactly the capacity, one over
    tape_append(&t, 1.0, 1);
    assert(t.tape_segs.size() == 1 && seg(0, 0, 1, 1.0, 0) && taped_steps(&t) == 1);
    assert(open_segment_room(&t, 1.0) == 3 && open_segment_room(&t, 2.0) == 0);                                    // room under the same dt, none under another
    assert(tape_slots_needed(&t, 1.0, 3) == 0 && tape_slots_needed(&t, 1.0, 4) == 1 && tape_slots_needed(&t, 2.0, 1) == 1);
    assert(tape_slots_needed(&t, 1.0, 3 + 8) == 2 && tape_slots_needed(&t, 1.0, 3 + 9) == 3);                      // 2 free slots: the capacity, one over
    tape_append(&t, 1.0, 2);                                                                                       // m < room + K, within the room
    assert(t.tape_segs.size() == 1 && seg(0, 0, 3, 1.0, 0) && open_segment_room(&t, 1.0) == 1);
    tape_append(&t, 1.0, 1 + 4);                                                                                   // m == room + K: fills, opens one full segment
    assert(t.tape_segs.size() == 2 && seg(0, 0, 4, 1.0, 0) && seg(1, 4, 4, 1.0, 1) && taped_steps(&t) == 8 && open_segment_room(&t, 1.0) == 0);
    tape_append(&t, 2.0, 3);                                                                                       // another dt: a new segment at once
    assert(t.tape_segs.size() == 3 && seg(2, 8, 3, 2.0, 2) && taped_steps(&t) == 11 && tape_slots_used(&t) == 3);
    assert(tape_slots_needed(&t, 2.0, 1) == 0 && tape_slots_needed(&t, 2.0, 2) == 1 && tape_slots_needed(&t, 1.0, 1) == 1);
    t.tape_segs.clear();
    t.tape_cap = 4;
    tape_append(&t, 1.0, 2);
    tape_append(&t, 1.0, 2 + 4 + 3);                                                                               // m > room + K: fills, a full segment, a part
    assert(t.tape_segs.size() == 3 && seg(0, 0, 4, 1.0, 0) && seg(1, 4, 4, 1.0, 1) && seg(2, 8, 3, 1.0, 2) && taped_steps(&t) == 11);
    tape_append(&t, 1.0, 0);
    assert(t.tape_segs.size() == 3 && taped_steps(&t) == 11);
    // ... and per step (K = 0): a slot per step, no segments
    trm_ctx p;
    p.tape_cap = 5;
    assert(taped_steps(&p) == 0 && open_segment_room(&p, 1.0) == 0 && tape_slots_needed(&p, 1.0, 5) == 5 && tape_slots_needed(&p, 1.0, 6) == 6);
    tape_append(&p, 1.0, 2);
    tape_append(&p, 2.0, 1);
    assert(p.tape_segs.empty() && p.tape_dt == std::vector<double>({1.0, 1.0, 2.0}) && taped_steps(&p) == 3 && tape_slots_used(&p) == 3);
    assert(tape_slots_needed(&p, 2.0, 2) == 2 && open_segment_room(&p, 2.0) == 0);
    std::puts("derivative preconditions ok");
    return 0;
}
