"""What the tests of soil-moisture records on the heat + Richards adjoint share (test_richards_record_host.py,
test_gpu_adjoint_richards_record.py): the cases, the records and the CPU reference.  Everything here is computed on the CPU; no figure
of the device enters.

The construction of tests/adjoint_record.py on tests/linearised_richards_params.py: LRP.run(..., nsteps = s) gives the Jacobian of state
s over the 2 Nz state seeds and the 7 parameter seeds, for every position s of the record.  The gradient of the misfit is the
np.longdouble sum over the record's samples of J_s[saturation, levels]^T (w (sat_s - sat_obs)), plus the contraction of J_n with the
final cotangents of the variant; S is the same sum over absolute values, e_ref the normalised difference of the float64 evaluation of
the same sums.

Groups (cases of richards_cases.CASES, each with a record):
  edges   Nz in {2, 3, 32, 33, 64} x 13 columns and 64 x 1, three hydraulics, both boundary sets, and the two repair cases, with the
          record at POSITIONS = (0, 3, 5, 6) on one_hot_levels(Nz): with six steps in launches of 4 and 2, positions 3 and 5 fall inside a
          launch, 0 is the last launch's last step and 6 is the fold's
  dense   positions 0 ... 6 on all levels: (3, 13) and (33, 13) with the default hydraulics (both boundary sets and the repair case) and
          (64, 1) generic -- every step of every launch, the first of a launch included, is observed, and every lane owns a sample
  ends    positions (0, 6) on the top level of (2, 13)
Variants: "record" (zero final cotangents) and "record+final" (the dense final cotangent of linearised_richards_params.cotangents).
Parts: "state" (gU, gsat), "params" (the seven per-column gradients) and "misfit loss".

Observations: the float64 restatement's saturation moved by 0.02 ... 0.08 either way, weights uniform in 0.5 ... 2, from a default_rng
seeded per case.

Bounds are derived: FACTOR (8) x the larger of the record contractions' own e_ref for the part and the e_ref the existing references
assign to the case -- richards_adjoint_cases.reference(case).e_ref for the state (and the loss: it is a function of the taped saturations),
the pooled e_ref behind linearised_richards_params.bound(case) for the parameters: the sweep's steps are the same steps, and that is the
rounding they carry.  The record's own parameter e_ref is pooled over the group's cases of one Nz and hydraulics, as LRP.pool does,
because a one-column case samples it once.  Ceilings: richards_adjoint_cases.BROKEN and linearised_richards_params.CEILING."""
import functools

import numpy as np

import linearised_richards as LR
import linearised_richards_params as LRP
import richards_adjoint_cases as RA
import richards_cases as RC
from richards_cases import DT, DZ, FACTOR, SPL, STEPS, case_id, one_hot_levels     # noqa: F401  (re-exported to the tests)

LD = np.longdouble
POSITIONS = (0, 3, 5, 6)
EDGE_SHAPES = ((2, 13), (3, 13), (32, 13), (33, 13), (64, 13), (64, 1))
VARIANTS = ("record", "record+final")
PARTS = ("state", "params", "misfit loss")
SAT = LR.FIELDS.index("saturation")
PARAMS = LRP.PARAMS


def _dense(case):
    Nz, Nh, hyd, _ = case
    return ((Nz, Nh) in ((3, 13), (33, 13)) and hyd == "default") or ((Nz, Nh) == (64, 1) and hyd == "generic")


GROUPS = {
    "edges": [c for c in RC.CASES if (c[0], c[1]) in EDGE_SHAPES],
    "dense": [c for c in RC.CASES if _dense(c)],
    "ends": [c for c in RC.CASES if (c[0], c[1]) == (2, 13)],
}
CASES = [(group, case) for group, cases in GROUPS.items() for case in cases]


def record_id(rcase):
    return f"{rcase[0]}-{case_id(rcase[1])}"


def positions_of(rcase):
    return {"edges": POSITIONS, "dense": tuple(range(STEPS + 1)), "ends": (0, STEPS)}[rcase[0]]


def levels_of(rcase):
    Nz = rcase[1][0]
    return {"edges": one_hot_levels(Nz), "dense": list(range(Nz)), "ends": [Nz - 1]}[rcase[0]]


def prefix(case, nsteps, dtype, inputs=None):
    """the restatement stopped after `nsteps` steps, seeded in the state and the parameters"""
    p, U0, sat, bcs = RC.inputs(case)[:4] if inputs is None else inputs
    return LRP.run([DZ] * case[0], U0, sat, bcs, p, DT, nsteps, dtype=dtype)


def make_record(rcase, sat_narrow):
    """{positions, levels, observed [npos][nlevels][Nh], weight}: sat_obs the float64 restatement's saturation moved by 0.02 ... 0.08
    either way, weights uniform in 0.5 ... 2"""
    rng = np.random.default_rng(7000 + CASES.index(rcase))
    observed, weight = [], []
    for s in sat_narrow:
        observed.append(s + rng.choice([-1.0, 1.0], s.shape) * rng.uniform(0.02, 0.08, s.shape))
        weight.append(rng.uniform(0.5, 2.0, s.shape))
    return dict(positions=list(positions_of(rcase)), levels=list(levels_of(rcase)), observed=np.stack(observed), weight=np.stack(weight))


def loss_float64(saturations, record):
    """the misfit per column as float64 forms it: positions in ascending order, levels in list order, one term at a time"""
    s = np.zeros(saturations[0].shape[1])
    for sat, obs, w in zip(saturations, record["observed"], record["weight"]):
        for j in range(obs.shape[0]):
            r = sat[j] - obs[j]
            s = s + 0.5 * w[j] * r * r
    return s


def final_cotangent(case, variant):
    """[5][Nz][Nh]: zero, or the dense final cotangent of the case"""
    dense = LRP.cotangents(case)["dense"]
    return dense if variant == "record+final" else np.zeros_like(dense)


class RecordReference:
    """The reference of a record case, computed once on the CPU.  `expected[(part, variant)]` = (ref, S) on the kept columns -- state:
    [2 Nz][kept], params: [7][kept], misfit loss: [kept] -- `parts[(part, variant)]` its e_ref, `identity[variant]` = (ref, S) of
    sum_k <w_k r_k, J_s v> + <final, J_n v> per kept column for the dense state seed v of the case.  `jacobians`: keep the
    extended-precision Jacobians of every position, all columns (the host test's consistency checks).  `record`: a record in place of
    the drawn one (positions and levels the case's)."""

    def __init__(self, rcase, jacobians=False, record=None):
        group, case = rcase
        self.rcase, self.case = rcase, case
        Nz = case[0]
        positions, levels = positions_of(rcase), levels_of(rcase)
        assert positions[-1] == STEPS
        wide = [prefix(case, s, LD) for s in positions]
        narrow = [prefix(case, s, np.float64) for s in positions]
        self.keep = keep = LR.kept_columns(wide[-1], narrow[-1])          # (the whole run: its prefixes are in its trajectory)
        self.sat_narrow = sat_narrow = [r.final["saturation"].x[levels].astype(np.float64) for r in narrow]
        sat_wide = [r.final["saturation"].x[levels] for r in wide]
        self.record = rec = make_record(rcase, sat_narrow) if record is None else record
        J_wide, J_narrow = [r.jacobian() for r in wide], [r.jacobian() for r in narrow]
        self.J = J_wide if jacobians else None
        # the rows no finite arithmetic reaches (a head at zero saturation: the repair cases' last state), as LRP.Reference leaves them out
        for k in range(len(positions)):
            nonfinite = ~(np.isfinite(J_wide[k].astype(np.float64)) & np.isfinite(J_narrow[k]))
            assert not nonfinite[SAT].any(), (record_id(rcase), "a saturation row is not finite")
            for variant in VARIANTS:
                if k == len(positions) - 1:
                    assert not np.any(nonfinite & (final_cotangent(case, variant) != 0)[:, :, None, :]), (record_id(rcase), "a cotangent on a non-finite row")
            J_wide[k], J_narrow[k] = np.where(nonfinite, LD(0), J_wide[k]), np.where(nonfinite, 0.0, J_narrow[k])
        with np.errstate(invalid="ignore"):
            self.cot_wide = [rec["weight"][k].astype(LD) * (sat_wide[k] - rec["observed"][k].astype(LD)) for k in range(len(positions))]
            cot_narrow = [rec["weight"][k] * (sat_narrow[k] - rec["observed"][k]) for k in range(len(positions))]
        gap = [~((rec["observed"][k] == rec["observed"][k]) & (rec["weight"][k] > 0.0)) for k in range(len(positions))]
        self.cot_wide = [np.where(g, LD(0), c) for g, c in zip(gap, self.cot_wide)]
        cot_narrow = [np.where(g, 0.0, c) for g, c in zip(gap, cot_narrow)]
        dU = RC.inputs(case)[4]
        self.expected, self.parts, self.identity = {}, {}, {}
        for variant in VARIANTS:
            final = final_cotangent(case, variant)
            # the terms of the loss: (Jacobian rows [rows][seeds][Nh] wide / narrow, cotangent wide / narrow [rows][Nh])
            terms = [(J_wide[-1].reshape((-1,) + J_wide[-1].shape[2:]), J_narrow[-1].reshape((-1,) + J_narrow[-1].shape[2:]),
                      final.reshape(-1, final.shape[-1]).astype(LD), final.reshape(-1, final.shape[-1]))]
            for k in range(len(positions)):
                terms.append((J_wide[k][SAT][levels], J_narrow[k][SAT][levels], self.cot_wide[k], cot_narrow[k]))
            ref = Ssum = got = 0
            for Jw, Jn, w_wide, w_narrow in terms:
                Jw, Jn, w_wide, w_narrow = Jw[..., keep], Jn[..., keep], w_wide[..., keep], w_narrow[..., keep]
                ref = ref + np.einsum("ijc,ic->jc", Jw.astype(LD), w_wide)
                Ssum = Ssum + np.einsum("ijc,ic->jc", np.abs(Jw).astype(LD), np.abs(w_wide))
                got = got + np.einsum("ijc,ic->jc", Jn.astype(LD), w_narrow.astype(LD))
            self._part(("state", variant), got[:2 * Nz], ref[:2 * Nz], Ssum[:2 * Nz])
            self._part(("params", variant), got[2 * Nz:], ref[2 * Nz:], Ssum[2 * Nz:])
            L_wide = sum(np.sum(np.where(g, LD(0), LD(0.5) * w.astype(LD) * (s - np.where(g, 0.0, obs).astype(LD)) ** 2), axis=0)
                         for s, obs, w, g in zip(sat_wide, rec["observed"], rec["weight"], gap))[keep]
            clean = dict(observed=[np.where(g, s, obs) for g, s, obs in zip(gap, sat_narrow, rec["observed"])],
                         weight=[np.where(g, 0.0, w) for g, w in zip(gap, rec["weight"])])
            self._part(("misfit loss", variant), loss_float64(sat_narrow, clean)[keep].astype(LD), L_wide, L_wide)
            v = dU[:, keep].astype(LD)
            self.identity[variant] = (np.einsum("jc,jc->c", ref[:2 * Nz], v), np.einsum("jc,jc->c", Ssum[:2 * Nz], np.abs(v)))
        self.e_ref = {part: max(self.parts[(part, variant)] for variant in VARIANTS) for part in PARTS}

    def _part(self, key, got, ref, Ssum):
        zero = Ssum == 0
        assert np.all(got[zero] == 0), (key, "a non-zero value where every product of the reference is zero")
        self.expected[key] = (ref, Ssum)
        self.parts[key] = 0.0 if zero.all() else float(np.max(np.abs(got - ref)[~zero] / Ssum[~zero]))

    def error(self, part, variant, dev):
        """|dev - ref| / S of the device's figures on the kept columns -- state: gU and gsat stacked [2 Nz][Nh], params: [7][Nh], misfit
        loss: [Nh]; exact zeros where S is zero"""
        ref, Ssum = self.expected[(part, variant)]
        dev = np.asarray(dev)[..., self.keep]
        zero = Ssum == 0
        assert np.all(dev[zero] == 0.0), (record_id(self.rcase), part, variant, "non-zero where the reference is exactly zero")
        return 0.0 if zero.all() else float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))


def schedule_reference(rcase, record, schedule):
    """(g_ref [2 Nz][kept], S, e_ref, kept columns) of the state part of the record alone, the run under a schedule [(dt, steps), ...]
    (richards_adjoint_cases.run_schedule, state seeds): the two-dt reference of the split tests"""
    case = rcase[1]
    p, U0, sat, bcs, _ = RC.inputs(case)
    levels = record["levels"]

    def stopped(s, dtype):
        cut, left = [], s
        for dt, steps in schedule:
            cut.append((dt, min(steps, left)))
            left -= min(steps, left)
        return RA.run_schedule([DZ] * case[0], U0, sat, bcs, p, cut, dtype)

    wide, narrow = [stopped(s, LD) for s in record["positions"]], [stopped(s, np.float64) for s in record["positions"]]
    keep = LR.kept_columns(wide[-1], narrow[-1])
    ref = Ssum = got = 0
    for k in range(len(wide)):
        Jw, Jn = wide[k].jacobian()[SAT][levels][..., keep], narrow[k].jacobian()[SAT][levels][..., keep]
        w_wide = (record["weight"][k].astype(LD) * (wide[k].final["saturation"].x[levels] - record["observed"][k].astype(LD)))[..., keep]
        w_narrow = (record["weight"][k] * (narrow[k].final["saturation"].x[levels].astype(np.float64) - record["observed"][k]))[..., keep]
        ref = ref + np.einsum("ijc,ic->jc", Jw.astype(LD), w_wide)
        Ssum = Ssum + np.einsum("ijc,ic->jc", np.abs(Jw).astype(LD), np.abs(w_wide))
        got = got + np.einsum("ijc,ic->jc", Jn.astype(LD), w_narrow.astype(LD))
    return ref, Ssum, float(np.max(np.abs(got - ref)[Ssum > 0] / Ssum[Ssum > 0])), keep


@functools.lru_cache(maxsize=None)
def reference(rcase):
    """shared by the tests of a case; nothing in it is modified later"""
    return RecordReference(rcase)


def pool(rcase):
    """the record cases whose parameter e_ref the bound of `rcase` is taken over: the group's cases of one Nz and hydraulics"""
    group, case = rcase
    if case[3] == "repair":
        return [rcase]
    return [(group, q) for q in GROUPS[group] if q[0] == case[0] and q[2] == case[2] and q[3] != "repair"]


def ceiling(part):
    return LRP.CEILING if part == "params" else RA.BROKEN


@functools.lru_cache(maxsize=None)
def bound(rcase, part):
    """FACTOR x the larger of the record's own e_ref of the part and the e_ref the existing references assign to the case, in
    (0, ceiling]"""
    case = rcase[1]
    if part == "params":
        own = max(reference(q).e_ref["params"] for q in pool(rcase))
        existing = LRP.bound(case) / FACTOR
    else:
        own = reference(rcase).e_ref[part]
        existing = RA.reference(case).e_ref
    b = FACTOR * max(own, existing)
    assert 0.0 < b <= ceiling(part), (record_id(rcase), part, "e_ref is no measurement of fp64 rounding", own, existing)
    return b
