"""Records the bounds of tests/hop_attention_ref.py and tests/hop_recursive_ref.py on every fixture and on a few
random cases into hop_bounds_before.npz.  It was run once on the modules as they were BEFORE the special-value
rules (0 * inf = 0 where the zero is exact) went in; test_hop_special_cpu.py holds today's modules to those
numbers at relative 1e-12, so a rule for special values can never move a bound on finite inputs.  Running it
again records today's bounds, which is only right after a deliberate change of the derivation.

    python tests/golden/make_hop_bounds.py [directory holding the two modules to record, default tests/]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RANDOM_ATTENTION = (("gate", 61, 6, 4, 1, 4, 100), ("ori_ref", 61, 3, 4, 1, 4, 101), ("jk", 61, 65, 4, 1, 4, 102),
                    ("jk", 300, 1, 5, 0, 5, 103))
RANDOM_RECURSIVE = ((61, 6, 5, 4, 200), (65, 4, 32, 32, 201), (300, 65, 3, 3, 202))
KEYS = ("E_P", "E_out", "E_dw", "E_db")


def bounds(R, RR):
    """{name__key: bound} of every fixture and random case, from the modules R (attention) and RR (recursive)."""
    out = {}
    za = np.load(os.path.join(HERE, "hop_attention.npz"), allow_pickle=False)
    for name in R.CASES:
        c, hops, w, b, C, *_ = R.load_case(za, name)
        out[name] = R.evaluate(c["kind"], hops, c["start"], c["end"], w, b, G=C)
    zr = np.load(os.path.join(HERE, "hop_recursive.npz"), allow_pickle=False)
    for name in RR.CASES:
        c, hops, w, b, C, *_ = RR.load_case(zr, name)
        out[name] = RR.evaluate(hops, c["end"], w, b, G=C)
    for kind, n, d, T, start, end, seed in RANDOM_ATTENTION:
        hops, w, b, C = R.random_case(kind, n, d, T, start, end, seed)
        out[f"random_{kind}_{seed}"] = R.evaluate(kind, hops, start, end, w, b, G=C)
    for n, d, T, end, seed in RANDOM_RECURSIVE:
        hops, w, b, C = RR.random_case(n, d, T, seed)
        out[f"random_recursive_{seed}"] = RR.evaluate(hops, end, w, b, G=C)
    return {f"{name}__{k}": np.asarray(ref[k], dtype=np.float64) for name, ref in out.items() for k in KEYS}


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(HERE))
    import hop_attention_ref
    import hop_recursive_ref
    np.savez_compressed(os.path.join(HERE, "hop_bounds_before.npz"), **bounds(hop_attention_ref, hop_recursive_ref))
