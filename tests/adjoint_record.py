"""What the tests of attached temperature records share (test_adjoint_record_host.py, test_gpu_adjoint_record.py): the cases, the records
and the CPU reference.

adjoint_observations.reference generalised to any list of positions and levels, with the same construction: linearised_heat.run(...,
nsteps = s) gives dX_s / d(input) for every position s of the record; the gradient of the misfit is the sum over the record's samples
(and the final cotangents of the case) of the contractions of those Jacobians with w (T_s - T_obs), in np.longdouble, S the same sum
over absolute values, e_ref the normalised difference of the float64 evaluation of the same sums.  The parts are "misfit gradient
state | boundary | params | series" and "misfit loss".

Three groups of cases, each a case of adjoint_observations.CASES with a record:
  AO      the 48 cases with the record of adjoint_observations.record_of at POSITIONS = (0, 3, 5, 6) on the levels 0, Nz - 1 (31, 32):
          positions 3 and 5 fall inside launches of up to 4 steps and inside segments of K = 4
  dense   positions 0 ... 6, all of them, on all Nz levels: (3, 13), (33, 13), (64, 1) with the three boundary sets and the seriesed
          one, rho_soc 26 -- every step of every launch is observed, every lane owns a sample
  ends    positions (0, 6) on the top level of (2, 13): nothing inside a launch but position 0, the fold takes the other
The final cotangents of the edge tests ride with every record."""
import functools

import numpy as np

import adjoint_observations as AO
from boundary_derivatives import LD
from test_gpu_derivative_edges import STEPS, Reference, blocks, case_id
from test_gpu_tangent import TANGENTS

DENSE_SHAPES = ((3, 13), (33, 13), (64, 1))
GROUPS = {
    "AO": [c for c in AO.CASES],
    "dense": [c for c in AO.CASES if (c[0], c[1]) in DENSE_SHAPES and c[4] == 26.0],
    "ends": [c for c in AO.CASES if (c[0], c[1]) == (2, 13) and c[4] == 26.0],
}
CASES = [(group, case) for group, cases in GROUPS.items() for case in cases]


def record_id(rcase):
    return f"{rcase[0]}-{case_id(rcase[1])}"


def positions_of(rcase):
    return {"AO": AO.POSITIONS, "dense": tuple(range(STEPS + 1)), "ends": (0, STEPS)}[rcase[0]]


def levels_of(rcase):
    Nz = rcase[1][0]
    return {"AO": AO.observed_levels(Nz), "dense": list(range(Nz)), "ends": [Nz - 1]}[rcase[0]]


def make_record(rcase, narrow):
    """{positions, levels, observed [npos][nlevels][Nh], weight}: the AO group has adjoint_observations' record; the others are drawn
    the same way -- T_obs the float64 restatement's temperature moved by 0.5 ... 1.5 K either way, weights of the magnitude of the final
    temperature cotangent"""
    group, case = rcase
    positions, levels = positions_of(rcase), levels_of(rcase)
    if group == "AO":
        rec = AO.record_of(case, narrow)
        observed, weight = rec["observed"], rec["weight"]
    else:
        rng = np.random.default_rng(9000 + CASES.index(rcase))
        observed, weight = [], []
        for result in narrow:
            T = result.value("temperature")[levels].astype(np.float64)
            observed.append(T + rng.choice([-1.0, 1.0], T.shape) * rng.uniform(0.5, 1.5, T.shape))
            weight.append(rng.uniform(0.5, 2.0, T.shape) * 3.0e6)
    return dict(positions=list(positions), levels=list(levels), observed=np.stack(observed), weight=np.stack(weight))


def loss_float64(temperatures, record):
    """the misfit per column as float64 forms it: positions in ascending order, levels in list order, one term at a time"""
    s = np.zeros(temperatures[0].shape[1])
    for T, obs, w in zip(temperatures, record["observed"], record["weight"]):
        for j in range(obs.shape[0]):
            r = T[j] - obs[j]
            s = s + 0.5 * w[j] * r * r
    return s


class RecordReference(Reference):
    """Reference of test_gpu_derivative_edges.py (error, bound) over "misfit gradient <input>" for every input and "misfit loss".
    `identity`: (ref, S) of sum_k <w_k, dT_k dU_0> + <final, dX_n dU_0> per column for the dense dU_0 of the case."""

    def __init__(self, rcase):
        group, case = rcase
        self.rcase, self.case = rcase, case
        self.inputs = AO.inputs(case)
        positions = positions_of(rcase)
        wide = [AO.prefix(case, s, LD) for s in positions]
        narrow = [AO.prefix(case, s, np.float64) for s in positions]
        assert positions[-1] == STEPS
        self.keep = keep = AO.LH.kept_columns(wide[-1], narrow[-1])     # (the whole run: its prefixes are in its trajectory)
        self.record = rec = make_record(rcase, narrow)
        levels = rec["levels"]
        J_wide, J_narrow = [blocks(r, case) for r in wide], [blocks(r, case) for r in narrow]
        final = self.inputs[5]["cotangents"]
        self.T_narrow = T_narrow = [r.value("temperature")[levels].astype(np.float64) for r in narrow]
        T_wide = [r.value("temperature")[levels] for r in wide]
        # the terms of the loss: (position index, rows of the fields or None for all, cotangent of the wide / the narrow evaluation)
        terms = [(len(positions) - 1, None, final.astype(LD), final)]
        for k in range(len(positions)):
            terms.append((k, levels, AO.misfit_cotangent(T_wide[k], rec["observed"][k], rec["weight"][k], LD),
                          AO.misfit_cotangent(T_narrow[k], rec["observed"][k], rec["weight"][k], np.float64)))
        self.expected, self.parts = {}, {}
        for key, axes in AO.AXES.items():
            if key not in J_wide[0]:
                continue
            ref = Ssum = got = 0
            for k, rows, w_wide, w_narrow in terms:
                Jw, Jn = J_wide[k][key][..., keep], J_narrow[k][key][..., keep]
                if rows is not None:
                    Jw, Jn = Jw[:, rows], Jn[:, rows]
                ref = ref + np.einsum(axes, Jw.astype(LD), w_wide[..., keep])
                Ssum = Ssum + np.einsum(axes, np.abs(Jw).astype(LD), np.abs(w_wide[..., keep]))
                got = got + np.einsum(axes, Jn.astype(LD), w_narrow[..., keep].astype(LD))
            self._part(f"misfit gradient {key}", got, ref, Ssum)
        L_wide = sum(np.sum(LD(0.5) * w.astype(LD) * (T - obs.astype(LD)) ** 2, axis=0) for T, obs, w in zip(T_wide, rec["observed"], rec["weight"]))[keep]
        self._part("misfit loss", loss_float64(T_narrow, rec)[keep].astype(LD), L_wide, L_wide)
        # the adjoint identity with the dense seed of the case
        dU = self.inputs[5]["state"]
        ref = Ssum = 0
        for k, rows, w_wide, _ in terms:
            Jw = J_wide[k]["state"][..., keep]
            if rows is not None:
                Jw = Jw[:, rows]
            ref = ref + np.einsum("xijc,xic,jc->c", Jw.astype(LD), w_wide[..., keep], dU[..., keep].astype(LD))
            Ssum = Ssum + np.einsum("xijc,xic,jc->c", np.abs(Jw).astype(LD), np.abs(w_wide[..., keep]), np.abs(dU[..., keep]).astype(LD))
        self.identity = (ref, Ssum)
        self.e_ref = max(self.parts.values())

    def _part(self, label, got, ref, Ssum):
        zero = Ssum == 0
        assert np.all(got[zero] == 0), (label, "a non-zero value where every product of the reference is zero")
        self.expected[label] = (ref, Ssum)
        self.parts[label] = 0.0 if zero.all() else float(np.max(np.abs(got - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(rcase):
    """shared by the tests of a case; nothing in it is modified later"""
    return RecordReference(rcase)
