"""What the tests of adjoint observations share (test_adjoint_observations_host.py, test_gpu_adjoint_observations.py): the cases, the
record and the CPU reference, built on test_gpu_derivative_edges.py and linearised_heat.py.

A loss that reads the run at the taped positions POSITIONS = 0 (before any step), 3 (inside what would be one launch of 4), 5 and 6
(the end, together with final cotangents) on the levels 0 and Nz - 1, plus 31 and 32 where the column has them.  Two kinds: linear --
a cotangent of each of U, T, liq on those levels at every position -- and misfit, 1/2 w (T - T_obs)^2 with T_obs between 0.5 K and
1.5 K off the model temperature and weights of the magnitude of the final temperature cotangent, so that no term hides behind
another in S.  The final cotangents of the edge tests ride with both.

The reference: linearised_heat.run(..., nsteps = s) gives dX_s / d(input) for every observed position s; the gradient of a kind is the
sum over its terms of the contractions of those Jacobians with the terms' cotangents, in np.longdouble, S the same sum over absolute
values, e_ref the normalised difference of the float64 evaluation of the same sum.  The misfit's cotangent is w (T_s - T_obs) of the
evaluation's own T.  The loss is a part like the others: the float64 sum in registration and list order against the extended one."""
import functools

import numpy as np

import linearised_heat as LH
import series_derivatives as S
from boundary_derivatives import HALOS, LD
from parameter_derivatives import RHO_SOC
from test_gpu_derivative_edges import DT, DZ, SETS, STEPS, Reference, blocks, inputs, one_hot_levels
from test_gpu_adjoint import cotangents
from test_gpu_tangent import TANGENTS

SHAPES = [(Nz, 13) for Nz in (2, 3, 32, 33, 64)] + [(64, 1)]
POSITIONS = (0, 3, 5, 6)
K = 4
SERIES_SET = "T_top+flux_bottom"        # the set that also runs with its top temperature driven by a series
KINDS = ("linear", "misfit")
AXES = {"state": "xijc,xic->jc", "boundary": "xipc,xic->pc", "params": "xiqc,xic->qc", "series": "xinc,xic->nc"}
assert POSITIONS[-1] == STEPS

# (Nz, Nh, boundary set, halo policy, rho_soc, time indexing of the series or None): the three sets and the seriesed one, each with
# both carbon densities; the halo policy and the indexing alternate
CASES = [(Nz, Nh, bcset, HALOS[(n + m + r) % 2], rho, S.FD_INDEXINGS[(n + r) % 3] if seriesed else None)
         for n, (Nz, Nh) in enumerate(SHAPES) for m, (bcset, seriesed) in enumerate([(b, False) for b in SETS] + [(SERIES_SET, True)])
         for r, rho in enumerate(RHO_SOC)]


def observed_levels(Nz):
    return one_hot_levels(Nz)


def prefix(case, nsteps, dtype):
    p, U0, sat, bcs, series, _ = inputs(case)
    return LH.run([DZ] * case[0], U0, sat, bcs, p, DT, nsteps, dtype=dtype, mirror=case[3] == "mirror", series=series)


def record_of(case, narrow):
    """The record of a case: per position the cotangents of the linear kind [3][nlevels][Nh], T_obs [nlevels][Nh] and the misfit's
    weights [nlevels][Nh].  T_obs is the float64 restatement's temperature moved by 0.5 ... 1.5 K either way: data, like any record."""
    Nz, Nh = case[0], case[1]
    levels = observed_levels(Nz)
    rng = np.random.default_rng(7000 + CASES.index(case))
    linear, observed, weight = [], [], []
    for k, result in enumerate(narrow):
        w = cotangents(Nz, Nh, 60 + k)
        linear.append(np.stack([w[x][levels] for x in TANGENTS]))
        T = result.value("temperature")[levels].astype(np.float64)
        observed.append(T + rng.choice([-1.0, 1.0], T.shape) * rng.uniform(0.5, 1.5, T.shape))
        weight.append(rng.uniform(0.5, 2.0, T.shape) * 3.0e6)
    return dict(levels=levels, linear=linear, observed=observed, weight=weight)


def misfit_cotangent(T, observed, weight, dtype):
    """[3][nlevels][Nh]: w (T - T_obs) on the temperature, in the arithmetic of the evaluation"""
    out = np.zeros((3,) + observed.shape, dtype=dtype)
    out[TANGENTS.index("temperature")] = weight.astype(dtype) * (T.astype(dtype) - observed.astype(dtype))
    return out


def loss_float64(temperatures, record):
    """the misfit per column as float64 forms it: observations in registration order, levels in list order, one term at a time"""
    s = np.zeros(temperatures[0].shape[1])
    for T, obs, w in zip(temperatures, record["observed"], record["weight"]):
        for j in range(obs.shape[0]):
            r = T[j] - obs[j]
            s = s + 0.5 * w[j] * r * r
    return s


class ObservationReference(Reference):
    """Reference of test_gpu_derivative_edges.py (error, bound) over "<kind> gradient <input>" for both kinds and every input, and
    "misfit loss".  `identity`: (ref, S) of sum_k <w_k, dX_k dU_0> per column for the dense dU_0 of the case, the linear kind."""

    def __init__(self, case):
        self.case = case
        self.inputs = inputs(case)
        wide = [prefix(case, s, LD) for s in POSITIONS]
        narrow = [prefix(case, s, np.float64) for s in POSITIONS]
        self.keep = keep = LH.kept_columns(wide[-1], narrow[-1])     # (the whole run: its prefixes are in its trajectory)
        self.regimes = np.stack(wide[-1].regimes)
        self.record = rec = record_of(case, narrow)
        levels = rec["levels"]
        J_wide, J_narrow = [blocks(r, case) for r in wide], [blocks(r, case) for r in narrow]
        final = self.inputs[5]["cotangents"]
        T_wide = [r.value("temperature")[levels] for r in wide]
        T_narrow = [r.value("temperature")[levels].astype(np.float64) for r in narrow]
        self.expected, self.parts = {}, {}
        for kind in KINDS:
            # the terms of the loss: (position index, rows of the fields or None for all, cotangent of the wide / the narrow evaluation)
            terms = [(len(POSITIONS) - 1, None, final.astype(LD), final)]
            for k in range(len(POSITIONS)):
                if kind == "linear":
                    terms.append((k, levels, rec["linear"][k].astype(LD), rec["linear"][k]))
                else:
                    terms.append((k, levels, misfit_cotangent(T_wide[k], rec["observed"][k], rec["weight"][k], LD),
                                  misfit_cotangent(T_narrow[k], rec["observed"][k], rec["weight"][k], np.float64)))
            for key, axes in AXES.items():
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
                self._part(f"{kind} gradient {key}", got, ref, Ssum)
        L_wide = sum(np.sum(LD(0.5) * w.astype(LD) * (T - obs.astype(LD)) ** 2, axis=0) for T, obs, w in zip(T_wide, rec["observed"], rec["weight"]))[keep]
        self._part("misfit loss", loss_float64(T_narrow, rec)[keep].astype(LD), L_wide, L_wide)
        # the adjoint identity of the linear kind with the dense seed of the case
        dU = self.inputs[5]["state"]
        ref = Ssum = 0
        for k, rows, w_wide, _ in [(len(POSITIONS) - 1, None, final.astype(LD), None)] + [(k, levels, rec["linear"][k].astype(LD), None) for k in range(len(POSITIONS))]:
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
def reference(case):
    """shared by the tests of a case; nothing in it is modified later"""
    return ObservationReference(case)
