// The host side of tangent records (trm_host.hpp, trm_launch_derivative.inl) on contexts built by hand: no GPU call.  The tables the
// kernel indexes, every refusal of the attach with its text, how trm_step_tangent cuts its launches at the last position, and the
// launcher's preconditions -- no launch may index the position table outside [0, last position].
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_launch_derivative.inl"
#include <cassert>
#include <cstdio>

static std::string last;
namespace trmh {
int fail(trm_ctx*, int code, const std::string& msg) {
    last = msg;
    return code;
}
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) {
    static LaunchArgs<NF> a{};
    return a;
}
}  // namespace trmh
using namespace trmh;

static bool refused(int rc, const char* text) { return rc == TRM_EINVAL && last.find(text) != std::string::npos; }

int main() {
    // ---- the tables as an attach builds them: row_of_level[Nz], then row_of_position[last + 1]
    auto tables = [](int Nz, std::vector<int> levels, std::vector<int> positions) {
        RecordTable t;
        t.levels = levels;
        t.positions = positions;
        record_table_build(t, Nz, tangent_record_limit(positions));
        assert(t.entries == tangent_record_limit(positions) + 1 && t.host.size() == (size_t)(Nz + t.entries));
        return t.host;
    };
    assert((tables(6, {0, 2, 5}, {0, 3, 5, 6}) == std::vector<int32_t>{0, -1, 1, -1, -1, 2, /* positions */ 0, -1, -1, 1, -1, 2, 3}));
    assert((tables(2, {1}, {0}) == std::vector<int32_t>{-1, 0, 0, -1}));       // (position 0 alone: the entry's sample, and a step that has none)
    assert((tables(1, {0}, {2}) == std::vector<int32_t>{0, -1, -1, 0}));       // (no sample at the entry)

    // ---- the attach on a context of Nz = 6, Nh = 5
    double dummy[4 * 3 * 5] = {};
    trm_ctx c;
    c.Nz = 6;
    c.Nh = 5;
    const int32_t positions[4] = {0, 3, 5, 6}, levels[3] = {0, 2, 5};
    const char* who = "trm_tangent_record_attach";
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 3, levels, who), "trm_tangent_record_attach: no tangent is open (trm_tangent_open)"));
    assert(refused(tangent_record_attached(&c, "trm_tangent_record_rewind"), "trm_tangent_record_rewind: no tangent is open (trm_tangent_open)"));
    c.d_tan[0] = dummy;
    assert(tangent_record_attach_ok(&c, 4, positions, 3, levels, who) == TRM_OK);
    assert(refused(tangent_record_attached(&c, "trm_tangent_record_detach"), "no record is attached (trm_tangent_record_attach)"));
    // counts and NULL pointers
    assert(refused(tangent_record_attach_ok(&c, 0, positions, 3, levels, who), "bad argument"));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 0, levels, who), "bad argument"));
    assert(refused(tangent_record_attach_ok(&c, 4, nullptr, 3, levels, who), "bad argument"));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 3, nullptr, who), "bad argument"));
    // positions
    const int32_t negative[2] = {-1, 2}, twice[3] = {0, 3, 3}, back[3] = {0, 4, 3};
    for (const int32_t* bad : {negative + 0, twice + 0, back + 0})
        assert(refused(tangent_record_attach_ok(&c, bad == negative ? 2 : 3, bad, 3, levels, who), "the positions are tangent-step counts >= 0, strictly increasing"));
    // levels
    const int32_t below[1] = {-1}, above[1] = {6}, same[2] = {2, 2}, down[2] = {3, 1};
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 1, below, who), "the levels are rows 0 ... 5 of the host layout, strictly increasing"));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 1, above, who), "the levels are rows 0 ... 5"));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 2, same, who), "strictly increasing"));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 2, down, who), "strictly increasing"));
    // nothing attached: every launch is the record-free kernel's, nothing is held
    assert(tangent_record_steps(&c, 4) == 0 && tangent_record_bytes(&c) == 0);
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "k: no record is attached, or its tables are not built"));

    // ---- what an attach leaves (trm_tangent_record_attach, trm_derivative_api.hip)
    record_table_attach(c.trec, 4, positions, 3, levels);
    record_table_build(c.trec, c.Nz, tangent_record_limit(c.trec.positions));
    assert(refused(tangent_record_attach_ok(&c, 4, positions, 3, levels, who), "a record is attached already (trm_tangent_record_detach)"));
    assert(tangent_record_attached(&c, "trm_tangent_record_detach") == TRM_OK);
    assert(tangent_record_bytes(&c) == 2 * 4 * 3 * 5 * 8 + (6 + 7) * 4);
    // the launcher without device arrays
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "no record is attached, or its tables are not built"));
    c.trec.d_tables = (double*)c.trec.host.data();
    c.d_trec[0] = dummy;
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "no record is attached, or its tables are not built"));
    c.d_trec[1] = dummy;
    assert(tangent_record_launch_ok(&c, 1, "k") == TRM_OK);
    // sample arrays of another shape than the attached one
    c.trec.nlevels = 2;
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "k: the sample arrays do not have the attached shape"));
    c.trec.nlevels = 3;
    c.trec.npos = 5;
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "the sample arrays do not have the attached shape"));
    c.trec.npos = 4;

    // ---- the launches of trm_step_tangent: up to 4 steps each, cut at the last position (6); every launch the launcher accepts reads
    // the entries start ... start + nsteps of a table of last + 1 entries, which the walk below does under the sanitizer
    const int32_t* rows = c.trec.host.data() + c.Nz;
    const int total = 11, spl = 4;
    std::vector<int> recorded_launches, free_launches, sampled;
    for (int n = 0, m; n < total; n += m) {
        m = std::min(spl, total - n);
        const int recorded = tangent_record_steps(&c, m);
        if (recorded) {
            m = recorded;
            assert(tangent_record_launch_ok(&c, m, "k") == TRM_OK);
            const TangentRecordArgs r = tangent_record_args(&c, c.trec_position);
            assert(r.row_of_level == c.trec.host.data() && r.row_of_position == rows + c.trec_position && r.nlevels == 3);
            assert(r.sample_entry == (c.trec_position == 0 ? 1 : 0) && r.T == dummy && r.dT == dummy);
            if (r.sample_entry && r.row_of_position[0] >= 0) sampled.push_back(r.row_of_position[0]);
            for (int s = 0; s < m; ++s)
                if (r.row_of_position[s + 1] >= 0) sampled.push_back(r.row_of_position[s + 1]);
            recorded_launches.push_back(m);
        } else free_launches.push_back(m);
        c.trec_position += m;
    }
    assert((recorded_launches == std::vector<int>{4, 2}) && (free_launches == std::vector<int>{4, 1}) && c.trec_position == total);
    assert((sampled == std::vector<int>{0, 1, 2, 3}));                                          // every row once, in order
    // behind the last position the launcher refuses: it would index past the table
    assert(tangent_record_steps(&c, 4) == 0);
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "k: the launch leaves the record's position table"));
    c.trec_position = 6;
    assert(tangent_record_launch_ok(&c, 0, "k") == TRM_OK && refused(tangent_record_launch_ok(&c, 1, "k"), "the launch leaves the record's position table"));
    c.trec_position = 3;
    assert(tangent_record_steps(&c, 50) == 3 && tangent_record_launch_ok(&c, 3, "k") == TRM_OK);
    assert(refused(tangent_record_launch_ok(&c, 4, "k"), "the launch leaves the record's position table"));
    assert(refused(tangent_record_launch_ok(&c, -1, "k"), "the launch leaves the record's position table"));
    c.trec_position = -1;
    assert(refused(tangent_record_launch_ok(&c, 1, "k"), "the launch leaves the record's position table"));
    // a rewind: the counter at 0, the entry is sampled again
    c.trec_position = 0;
    assert(tangent_record_steps(&c, 1) == 1 && tangent_record_args(&c, 0).sample_entry == 1);
    // the seeds a ride needs are asked for first, as in the record-free launcher
    assert(tangent_seeds_ok<RIDE_NONE>(&c, 1, "k") == TRM_OK && tangent_seeds_ok<RIDE_BC>(&c, 1, "k") == TRM_EINVAL);
    // a record of position 0 alone: the launch that samples the entry runs one step, which has no sample
    trm_ctx z;
    z.Nz = 2;
    z.Nh = 1;
    const int32_t entry[1] = {0}, top[1] = {1};
    record_table_attach(z.trec, 1, entry, 1, top);
    record_table_build(z.trec, z.Nz, tangent_record_limit(z.trec.positions));
    assert(z.trec.entries == 2);
    z.trec.d_tables = (double*)z.trec.host.data();
    z.d_trec[0] = z.d_trec[1] = dummy;
    assert(tangent_record_steps(&z, 3) == 1 && tangent_record_launch_ok(&z, 1, "k") == TRM_OK && tangent_record_bytes(&z) == 2 * 8 + (2 + 2) * 4);
    const TangentRecordArgs rz = tangent_record_args(&z, 0);
    assert(rz.sample_entry == 1 && rz.row_of_position[0] == 0 && rz.row_of_position[1] == -1);
    assert(refused(tangent_record_launch_ok(&z, 2, "k"), "the launch leaves the record's position table"));
    z.trec_position = 1;
    assert(tangent_record_steps(&z, 3) == 0);
    std::printf("tangent record preconditions ok\n");
    return 0;
}
