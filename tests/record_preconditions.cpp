// The host-side bookkeeping of attached temperature records (trm_host.hpp) on contexts built by hand: no GPU call.  The level and
// position tables the backward kernels index and the RecordTable that holds them (shared with the tangent records), the slot counting of the checkpointed tape with a record attached (no position closes a
// segment), and every refusal of the attach, the mixing rules, the sweep and the downloads with its text.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_host.hpp"
#include <cassert>
#include <cmath>
#include <cstdio>

static std::string last;
namespace trmh {
int fail(trm_ctx*, int code, const std::string& msg) {
    last = msg;
    return code;
}
}  // namespace trmh
using namespace trmh;

static bool refused(int rc, const char* text) { return rc == TRM_EINVAL && last.find(text) != std::string::npos; }

int main() {
    // ---- the tables
    const std::vector<int32_t> lv = record_level_table(6, {0, 2, 5});
    assert((lv == std::vector<int32_t>{0, -1, 1, -1, -1, 2}));
    assert((record_level_table(3, {0, 1, 2}) == std::vector<int32_t>{0, 1, 2}));
    const std::vector<int32_t> pos = record_position_table(6, {0, 3, 5, 6});
    assert((pos == std::vector<int32_t>{0, -1, -1, 1, -1, 2, 3}));
    assert((record_position_table(0, {0}) == std::vector<int32_t>{0}));                  // (an empty tape: position 0 = n, the fold's)
    assert((record_position_table(2, {1, 4}) == std::vector<int32_t>{-1, 0, -1}));       // (a position behind the tape has no entry)
    // a launch over the steps [begin, end) reads the entries begin ... end: all inside the n + 1 of the table
    for (int begin = 0; begin <= 6; ++begin)
        for (int end = begin; end <= 6; ++end) assert((size_t)end < pos.size());

    // ---- a context with an open adjoint (any non-null cotangent pointer) of Nz = 6, Nh = 5
    double dummy = 0.0;
    trm_ctx c;
    c.Nz = 6;
    c.Nh = 5;
    const int32_t positions[4] = {0, 3, 5, 6}, levels[3] = {0, 2, 5};
    std::vector<double> observed(4 * 3 * 5, 1.0), weight(4 * 3 * 5, 2.0);
    const char* who = "trm_adjoint_observe_record";
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), weight.data(), who), "trm_adjoint_observe_record: no adjoint is open (trm_adjoint_open)"));
    assert(refused(record_results_ok(&c, &dummy, "trm_adjoint_record_misfit_download"), "no adjoint is open (trm_adjoint_open)"));
    c.d_adj[0] = &dummy;
    assert(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), weight.data(), who) == TRM_OK);
    assert(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), nullptr, who) == TRM_OK);
    // counts and NULL pointers
    assert(refused(record_attach_ok(&c, 0, positions, 3, levels, observed.data(), nullptr, who), "bad argument"));
    assert(refused(record_attach_ok(&c, 4, positions, 0, levels, observed.data(), nullptr, who), "bad argument"));
    assert(refused(record_attach_ok(&c, 4, nullptr, 3, levels, observed.data(), nullptr, who), "bad argument"));
    assert(refused(record_attach_ok(&c, 4, positions, 3, nullptr, observed.data(), nullptr, who), "bad argument"));
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, nullptr, nullptr, who), "bad argument"));
    // positions
    const int32_t negative[2] = {-1, 2}, twice[3] = {0, 3, 3}, back[3] = {0, 4, 3};
    for (const int32_t* bad : {negative + 0, twice + 0, back + 0})
        assert(refused(record_attach_ok(&c, bad == negative ? 2 : 3, bad, 3, levels, observed.data(), nullptr, who), "the positions are taped-step counts >= 0, strictly increasing"));
    // levels
    const int32_t below[1] = {-1}, above[1] = {6}, same[2] = {2, 2}, down[2] = {3, 1};
    assert(refused(record_attach_ok(&c, 4, positions, 1, below, observed.data(), nullptr, who), "the levels are rows 0 ... 5 of the host layout, strictly increasing"));
    assert(refused(record_attach_ok(&c, 4, positions, 1, above, observed.data(), nullptr, who), "the levels are rows 0 ... 5"));
    assert(refused(record_attach_ok(&c, 4, positions, 2, same, observed.data(), nullptr, who), "strictly increasing"));
    assert(refused(record_attach_ok(&c, 4, positions, 2, down, observed.data(), nullptr, who), "strictly increasing"));
    // host weights: the last one is checked too
    weight.back() = -1.0;
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), weight.data(), who), "a weight is negative or NaN"));
    weight.back() = std::nan("");
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), weight.data(), who), "a weight is negative or NaN"));
    weight.back() = 0.0;                                                                  // (a weight 0 is a gap, not an error)
    assert(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), weight.data(), who) == TRM_OK);
    // the mixing rules, either way
    c.observations.push_back(trm_ctx::Observation{0, TRM_ADJOINT_TEMPERATURE, 1, 1, nullptr});
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), nullptr, who), "per-position observations are registered"));
    assert(last.find("the two paths do not mix") != std::string::npos);
    c.observations.clear();
    assert(record_excludes_observations(&c, "trm_adjoint_observe") == TRM_OK);
    // ---- what an attach leaves (attach_record, trm_derivative_api.hip), and what follows from it
    record_table_attach(c.rec, 4, positions, 3, levels);
    assert(c.rec.npos == 4 && c.rec.nlevels == 3 && c.rec.entries == 0 && c.rec.host.empty());
    assert(refused(record_attach_ok(&c, 4, positions, 3, levels, observed.data(), nullptr, who), "a record is attached already (trm_adjoint_record_detach)"));
    assert(refused(record_excludes_observations(&c, "trm_adjoint_observe"), "trm_adjoint_observe: a temperature record is attached"));
    assert(refused(record_excludes_observations(&c, "trm_adjoint_observe_misfit"), "the two paths do not mix"));
    // downloads before a sweep
    assert(refused(record_results_ok(&c, &dummy, "trm_adjoint_record_residual_download"), "no sweep has run with this record (trm_adjoint_backward)"));
    assert(refused(record_results_ok(&c, nullptr, "trm_adjoint_record_residual_download"), "bad argument"));
    c.rec_swept = true;
    assert(record_results_ok(&c, &dummy, "trm_adjoint_record_residual_download") == TRM_OK);
    // what the library holds: residuals + misfit + the level table; its copies of a host record; the position table once it is built
    const int64_t cells = 4 * 3 * 5 * 8;
    assert(record_bytes(&c) == cells + 5 * 8 + 6 * 4);
    c.d_rec_owned = &dummy;
    assert(record_bytes(&c) == 2 * cells + 5 * 8 + 6 * 4);
    c.d_rec_weight = &dummy;
    record_table_build(c.rec, c.Nz, 6);
    assert(record_bytes(&c) == 3 * cells + 5 * 8 + (6 + 7) * 4);
    c.d_rec_owned = nullptr;
    // ---- slot counting: K = 4, the run of the tests in the pieces 3 + 2 + 1 -- no position closes a segment
    c.ckpt_interval = 4;
    c.tape_cap = 2;
    const double dt = 300.0;
    assert(tape_slots_needed(&c, dt, 6) == 2);
    assert(refused(record_fits_tape(&c, taped_steps(&c), "trm_adjoint_backward"), "the attached record is longer than the tape: position 6 of 0 taped steps"));
    tape_append(&c, dt, 3);
    assert(!c.tape_seg_closed && open_segment_room(&c, dt) == 1 && tape_slots_needed(&c, dt, 2) == 1);
    tape_append(&c, dt, 2);
    assert(!c.tape_seg_closed && tape_slots_used(&c) == 2 && tape_slots_needed(&c, dt, 1) == 0);
    assert(refused(record_fits_tape(&c, taped_steps(&c), "trm_adjoint_backward"), "position 6 of 5 taped steps"));
    tape_append(&c, dt, 1);
    assert(taped_steps(&c) == 6 && tape_slots_used(&c) == 2 && c.tape_segs[0].len == 4 && c.tape_segs[1].first == 4 && c.tape_segs[1].len == 2);
    assert(record_fits_tape(&c, taped_steps(&c), "trm_adjoint_backward") == TRM_OK);
    // a dense record on 24 steps, K = 8: three slots
    trm_ctx d;
    d.ckpt_interval = 8;
    d.rec.npos = 25;
    for (int p = 0; p <= 24; ++p) d.rec.positions.push_back(p);
    assert(tape_slots_needed(&d, dt, 24) == 3);
    tape_append(&d, dt, 24);
    assert(tape_slots_used(&d) == 3 && record_fits_tape(&d, taped_steps(&d), "trm_adjoint_backward") == TRM_OK);
    // without a record: nothing to refuse, nothing held
    trm_ctx e;
    assert(record_fits_tape(&e, 0, "trm_adjoint_backward") == TRM_OK && record_bytes(&e) == 0);
    e.d_adj[0] = &dummy;
    assert(refused(record_results_ok(&e, &dummy, "trm_adjoint_record_misfit_download"), "no record is attached (trm_adjoint_observe_record)"));
    // ---- the position table both records share (RecordTable), at the smallest shapes: Nz = 2 with one level.  The device copy is stood
    // in for by a host copy made where record_tables (trm_derivative_api.hip) uploads, so every read below is a read the sanitizer sees
    trm_ctx s;
    s.Nz = 2;
    s.Nh = 1;
    s.d_adj[0] = &dummy;
    const int32_t top[1] = {1}, ends[2] = {0, 3};
    assert(record_attach_ok(&s, 2, ends, 1, top, observed.data(), nullptr, who) == TRM_OK);
    record_table_attach(s.rec, 2, ends, 1, top);
    assert(record_bytes(&s) == 2 * 8 + 8 + 2 * 4 && !record_table_covers(s.rec, 0, 0));           // (no position entry before the first sweep)
    // a sweep over a tape of 3 steps: the record's last position is the tape's length
    assert(record_fits_tape(&s, 3, "trm_adjoint_backward") == TRM_OK);
    record_table_build(s.rec, s.Nz, 3);
    assert(s.rec.entries == 4 && (s.rec.host == std::vector<int32_t>{-1, 0, /* positions */ 0, -1, -1, 1}) && record_bytes(&s) == 2 * 8 + 8 + (2 + 4) * 4);
    std::vector<int32_t> device3 = s.rec.host;
    s.rec.d_tables = (double*)device3.data();
    assert(record_row_of_level(s.rec)[1] == 0 && record_row_of_position(s.rec, s.Nz, 0)[0] == 0 && record_row_of_position(s.rec, s.Nz, 3)[0] == 1);
    assert(record_table_covers(s.rec, 0, 3) && record_table_covers(s.rec, 3, 0) && record_table_covers(s.rec, 1, 2));
    assert(!record_table_covers(s.rec, 0, 4) && !record_table_covers(s.rec, 4, 0) && !record_table_covers(s.rec, -1, 1) && !record_table_covers(s.rec, 0, -1));
    // a second sweep, over 5 steps: built again.  The staging copy is replaced, which is why record_tables waits for the stream on either
    // side of its upload; the copy the device holds is untouched until the caller releases it
    s.rec.d_tables = nullptr;
    record_table_build(s.rec, s.Nz, 5);
    assert(s.rec.entries == 6 && s.rec.host.size() == 2 + 6 && (device3 == std::vector<int32_t>{-1, 0, 0, -1, -1, 1}));
    std::vector<int32_t> device5 = s.rec.host;
    s.rec.d_tables = (double*)device5.data();
    assert(record_table_covers(s.rec, 0, 5) && !record_table_covers(s.rec, 0, 6) && record_row_of_position(s.rec, s.Nz, 0)[3] == 1 && record_row_of_position(s.rec, s.Nz, 5)[0] == -1);
    // drop, then a second attach: a record of position 0 alone on a tape of 0 steps -- one entry, the fold's
    s.rec.d_tables = nullptr;
    assert(refused(record_attach_ok(&s, 1, ends, 1, top, observed.data(), nullptr, who), "a record is attached already"));
    record_table_drop(s.rec);
    assert(s.rec.npos == 0 && s.rec.nlevels == 0 && s.rec.entries == 0 && s.rec.host.empty() && s.rec.positions.empty() && s.rec.levels.empty() && record_bytes(&s) == 0);
    assert(record_attach_ok(&s, 1, ends, 1, top, observed.data(), nullptr, who) == TRM_OK);
    record_table_attach(s.rec, 1, ends, 1, top);
    assert(record_fits_tape(&s, 0, "trm_adjoint_backward") == TRM_OK);
    record_table_build(s.rec, s.Nz, 0);
    assert(s.rec.entries == 1 && (s.rec.host == std::vector<int32_t>{-1, 0, 0}) && record_table_covers(s.rec, 0, 0) && !record_table_covers(s.rec, 0, 1));
    std::printf("record preconditions ok\n");
    return 0;
}
