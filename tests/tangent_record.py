"""What the tests of tangent records share (test_tangent_record_host.py, test_gpu_tangent_record.py): the cases and the CPU reference.

The cases, positions and levels are adjoint_record.py's (AO: the 48 cases of adjoint_observations.py at the positions 0, 3, 5, 6; dense:
every position 0 ... 6 on every level of (3, 13), (33, 13), (64, 1); ends: positions 0 and 6 on the top level of (2, 13)).  For every
position s of a record, adjoint_observations.prefix(case, s, dtype) gives X_s and dX_s / d(input); the reference of a tangent record is
the temperature rows of those Jacobians at the record's levels, contracted with the seeds of the case -- the dense state seed, the
boundary seeds (cases without a series), the parameter seeds, the node seeds (cases with a series) -- stacked over the positions:
[npos][nlevels][Nh].  ref and S in np.longdouble, e_ref the normalised difference of the float64 Jacobian's contraction
(linearised_heat.contraction_error).  The temperature samples themselves are a part too, normalised by the contraction of the same
Jacobians with the magnitudes of the run's own inputs (below).

The adjoint identity: with the record (observed, weight) adjoint_record.make_record draws for the case, sum_k sum_i w r (J_k v)_i per
column, r = T_k - observed, is <gradient of the misfit, v> for every family of seeds: the parts "identity <input>"."""
import functools

import numpy as np

import adjoint_observations as AO
import adjoint_record as AR
import linearised_heat as LH
from boundary_derivatives import LD, PAIRS
from test_gpu_derivative_edges import SERIES_PAIR, Reference, blocks
from test_gpu_tangent import TANGENTS

CASES = AR.CASES
record_id = AR.record_id
positions_of, levels_of = AR.positions_of, AR.levels_of
T_ROW = TANGENTS.index("temperature")
# input -> (axes of the tangent contraction over the stacked positions, axes of the identity's)
AXES = {"state": ("kijc,jc->kic", "kijc,kic,jc->c"), "boundary": ("kipc,pc->kic", "kipc,kic,pc->c"), "params": ("kiqc,q->kic", "kiqc,kic,q->c"),
        "series": ("kinc,nc->kic", "kinc,kic,nc->c")}


def seed_keys(case):
    """the families of seeds a case is run with: a seriesed pair takes node seeds, and no per-column boundary seed"""
    return ("state", "series", "params") if case[5] else ("state", "boundary", "params")


class TangentRecordReference(Reference):
    """Reference of test_gpu_derivative_edges.py (error, bound) over "dT <input>" for every family of seeds, "temperature", and
    "identity <input>" ([Nh] each, with `record` = {positions, levels, observed, weight})."""

    def __init__(self, rcase):
        group, case = rcase
        self.rcase, self.case = rcase, case
        self.inputs = AO.inputs(case)
        vectors = self.inputs[5]
        positions, levels = positions_of(rcase), levels_of(rcase)
        wide = [AO.prefix(case, s, LD) for s in positions]
        narrow = [AO.prefix(case, s, np.float64) for s in positions]
        self.keep = keep = LH.kept_columns(wide[-1], narrow[-1])        # (the whole run: its prefixes are in its trajectory)
        self.record = rec = AR.make_record(rcase, narrow)
        T_wide = np.stack([r.value("temperature")[levels] for r in wide])[..., keep]
        T_narrow = np.stack([r.value("temperature")[levels].astype(np.float64) for r in narrow])[..., keep]
        # the temperature rows of every Jacobian at the record's levels, stacked over the positions: [npos][nlevels][inputs][Nh]
        J_wide, J_narrow = [blocks(r, case) for r in wide], [blocks(r, case) for r in narrow]
        self.expected, self.parts = {}, {}
        w_wide = rec["weight"][..., keep].astype(LD) * (T_wide - rec["observed"][..., keep].astype(LD))
        w_narrow = (rec["weight"][..., keep] * (T_narrow - rec["observed"][..., keep])).astype(LD)
        for key in seed_keys(case):
            Jw = np.stack([J[key][T_ROW][levels] for J in J_wide])[..., keep]
            Jn = np.stack([J[key][T_ROW][levels] for J in J_narrow])[..., keep]
            v = vectors[key][..., keep] if vectors[key].ndim > 1 else vectors[key]
            err, ref, Ssum = LH.contraction_error(Jn, Jw, v, AXES[key][0])
            self.expected[f"dT {key}"], self.parts[f"dT {key}"] = (ref, Ssum), err
            # the identity: the residuals of the evaluation's own temperatures
            ref = np.einsum(AXES[key][1], Jw.astype(LD), w_wide, np.asarray(v).astype(LD))
            Ssum = np.einsum(AXES[key][1], np.abs(Jw).astype(LD), np.abs(w_wide), np.abs(np.asarray(v)).astype(LD))
            got = np.einsum(AXES[key][1], Jn.astype(LD), w_narrow, np.asarray(v).astype(LD))
            self._part(f"identity {key}", got, ref, Ssum)
        # The temperature itself, on the scale of what forms it: S = sum_j |dT_s/dU_0j| (|U_0j| + L_theta_j) + sum_p |dT_s/db_p| |b_p|
        # (+ the same over the nodes of a series) -- the contraction of the same Jacobians with the magnitudes of the run's own inputs
        # (L_theta: the offset the frozen closure adds to U).  In phase change the rows are zero, S with them, and the sample must be 0.0.
        _, U0, _, bcs, series, _ = self.inputs
        Lth = np.broadcast_to(wide[-1].Ltheta, U0.shape)
        J_T = {key: np.abs(np.stack([J[key][T_ROW][levels] for J in J_wide])[..., keep]).astype(LD) for key in ("state", "boundary") + (("series",) if case[5] else ())}
        S_T = np.einsum(AXES["state"][0], J_T["state"], (np.abs(U0).astype(LD) + Lth)[..., keep])
        b = np.stack([np.abs(bcs[pair][1]) if pair in bcs else np.zeros(case[1]) for pair in PAIRS]).astype(LD)
        S_T = S_T + np.einsum(AXES["boundary"][0], J_T["boundary"], b[..., keep])
        if case[5]:
            S_T = S_T + np.einsum(AXES["series"][0], J_T["series"], np.abs(series[SERIES_PAIR[case[2]]][2]).astype(LD)[..., keep])
        self._part("temperature", T_narrow.astype(LD), T_wide, S_T)
        self.e_ref = max(self.parts.values())

    def _part(self, label, got, ref, Ssum):
        zero = Ssum == 0
        assert np.all(got[zero] == 0), (label, "a non-zero value where every product of the reference is zero")
        self.expected[label] = (ref, Ssum)
        self.parts[label] = 0.0 if zero.all() else float(np.max(np.abs(got - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(rcase):
    """shared by the tests of a case; nothing in it is modified later"""
    return TangentRecordReference(rcase)
