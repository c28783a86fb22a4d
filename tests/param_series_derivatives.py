"""What the tests of thermal-parameter derivatives of runs driven by boundary time series share (test_param_series_host.py,
test_gpu_param_series_edges.py): the cases and the CPU reference, both built on test_gpu_derivative_edges.py and linearised_heat.py.

Cases: the 36 series cases of test_gpu_derivative_edges.py, each with rho_soc 0 and 26 (an organic fraction of 0.2: the organic
parameters have non-zero blocks).  The reference of a case holds every product of the extended-precision Jacobian the device is asked
for -- dense and one-hot state tangents, boundary, parameter and node tangents, the four gradients -- and the joint tangent, whose
reference and S are the sums over its parts: |sum (got - ref)| / sum S cannot exceed the largest part's e_ref."""
import functools

import numpy as np

import linearised_heat as LH
from boundary_derivatives import LD, PAIRS
from parameter_derivatives import PARAMS, RHO_SOC
from test_gpu_derivative_edges import SERIES_CASES, SERIES_PAIR, Reference, blocks, inputs, one_hot_levels, restatement

CASES = [(Nz, Nh, bcset, halo, rho, indexing) for (Nz, Nh, bcset, halo, _, indexing) in SERIES_CASES for rho in RHO_SOC]
JOINT_PARTS = ("tangent dense", "tangent series", "tangent boundary", "tangent params")
ORGANIC = [PARAMS.index("k_organic"), PARAMS.index("c_organic")]


def contractions(case, vectors):
    """{label: (input, vector, einsum axes)}: every product of the Jacobian the device is asked for (the joint tangent is their sum)"""
    Nz, Nh = case[0], case[1]
    out = {"tangent dense": ("state", vectors["state"], "xijc,jc->xic")}
    for j in one_hot_levels(Nz):
        e = np.zeros((Nz, Nh))
        e[j] = 1.0
        out[f"tangent one-hot {j}"] = ("state", e, "xijc,jc->xic")
    w = vectors["cotangents"]
    out["tangent series"] = ("series", vectors["series"], "xinc,nc->xic")
    out["tangent boundary"] = ("boundary", vectors["boundary"], "xipc,pc->xic")
    out["tangent params"] = ("params", vectors["params"], "xiqc,q->xic")
    out["gradient state"] = ("state", w, "xijc,xic->jc")
    out["gradient series"] = ("series", w, "xinc,xic->nc")
    out["gradient boundary"] = ("boundary", w, "xipc,xic->pc")
    out["gradient params"] = ("params", w, "xiqc,xic->qc")
    return out


def other_pairs(case):
    """the pairs whose per-column seed / gradient the device holds: every pair but the seriesed one"""
    return [pair for pair in PAIRS if pair != SERIES_PAIR[case[2]]]


class ParamSeriesReference(Reference):
    """Reference of test_gpu_derivative_edges.py (error, bound) over the products above; `organic`: the largest |J| of the blocks of
    k_organic and c_organic; `joint_ceiling`: the largest e_ref among the parts of the joint tangent"""

    def __init__(self, case):
        self.case = case
        self.inputs = inputs(case)
        wide, narrow = restatement(case, LD), restatement(case, np.float64)
        self.keep = LH.kept_columns(wide, narrow)
        self.regimes = np.stack(wide.regimes)
        J_wide, J_narrow = blocks(wide, case), blocks(narrow, case)
        self.organic = float(np.max(np.abs(J_wide["params"][:, :, ORGANIC, :])))
        self.expected, self.parts = {}, {}
        got = {}
        for label, (key, v, axes) in contractions(case, self.inputs[5]).items():
            vk = v[..., self.keep] if v.ndim > 1 else v
            err, ref, Ssum = LH.contraction_error(J_narrow[key][..., self.keep], J_wide[key][..., self.keep], vk, axes)
            self.expected[label], self.parts[label] = (ref, Ssum), err
            if label in JOINT_PARTS:
                got[label] = np.einsum(axes, J_narrow[key][..., self.keep].astype(LD), np.asarray(vk).astype(LD))
        ref = sum(self.expected[label][0] for label in JOINT_PARTS)
        Ssum = sum(self.expected[label][1] for label in JOINT_PARTS)
        joint = sum(got[label] for label in JOINT_PARTS)
        zero = Ssum == 0
        assert np.all(joint[zero] == 0)
        self.expected["tangent joint"] = (ref, Ssum)
        self.parts["tangent joint"] = 0.0 if zero.all() else float(np.max(np.abs(joint - ref)[~zero] / Ssum[~zero]))
        self.joint_ceiling = max(self.parts[label] for label in JOINT_PARTS)
        self.e_ref = max(self.parts.values())


@functools.lru_cache(maxsize=None)
def reference(case):
    """shared by the tests of a case; nothing in it is modified later"""
    return ParamSeriesReference(case)
