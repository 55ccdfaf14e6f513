"""Generator of tests/golden/unit_spline_coupling.npz: inputs and outputs of the reference's
`unconstrained_rational_quadratic_spline` with per-element parameters, forward and inverse, in fp64.

    python tests/golden/make_golden_spline_coupling.py <path of the reference checkout> [output.npz]

Cases K in {2, 5, 8, 16}, 256 elements each, tail_bound 3: random points (about a tenth outside the tails), points exactly on
+-tail_bound and points exactly on interior knots (of the widths for the forward, of the heights for the inverse).  Only data
is recorded: `x`, `uw`, `uh`, `ud`, the forward outputs `z`, `lad`, the inverse inputs `zi` and the inverse outputs `xi`, `ladi`
(`ladi` as the reference returns it: the log-derivative of the inverse map)."""
import importlib.util
import os
import sys

import numpy as np
import torch

TAIL_BOUND = 3.0
CASES = (2, 5, 8, 16)
N = 256


def load_reference(root):
    path = os.path.join(root, "contextflow", "layers", "splines", "rational_quadratic.py")
    spec = importlib.util.spec_from_file_location("reference_rational_quadratic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root, out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from tests import spline_coupling_ref as ref
    rq = load_reference(root)
    data = {"tail_bound": np.float64(TAIL_BOUND), "cases": np.array(CASES)}
    for K in CASES:
        g = torch.Generator().manual_seed(1000 + K)
        uw = 1.5 * torch.randn(N, K, generator=g, dtype=torch.float64)
        uh = 1.5 * torch.randn(N, K, generator=g, dtype=torch.float64)
        ud = 1.5 * torch.randn(N, K - 1, generator=g, dtype=torch.float64)
        x = 2.0 * torch.randn(N, generator=g, dtype=torch.float64)
        x = x * (TAIL_BOUND / x.abs().quantile(0.9))                 # about a tenth outside the tails
        zi = 2.0 * torch.randn(N, generator=g, dtype=torch.float64)
        zi = zi * (TAIL_BOUND / zi.abs().quantile(0.9))
        cw, ch, _ = ref.knots(torch.cat([uw, uh, ud], -1), K, TAIL_BOUND)
        x[:4] = torch.tensor([TAIL_BOUND, -TAIL_BOUND, TAIL_BOUND, -TAIL_BOUND], dtype=torch.float64)
        zi[:4] = x[:4]
        for i in range(4, 36):                                       # exactly on interior knots
            k = 1 + (i % (K - 1))
            x[i] = cw[i, k]
            zi[i] = ch[i, k]
        call = lambda v, inv: rq.unconstrained_rational_quadratic_spline(
            v.clone(), uw.clone(), uh.clone(), ud.clone(), inverse=inv, tails="linear", tail_bound=TAIL_BOUND)
        z, lad = call(x, False)
        xi, ladi = call(zi, True)
        for name, t in (("x", x), ("uw", uw), ("uh", uh), ("ud", ud), ("z", z), ("lad", lad), ("zi", zi), ("xi", xi), ("ladi", ladi)):
            data["K%d_%s" % (K, name)] = t.numpy()
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "unit_spline_coupling.npz"))
