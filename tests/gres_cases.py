"""The stage-1 block cases shared by scripts/make_gres_golden.py and the gres tests (smallest shapes at which the kernels can
still go wrong: H != W, channel counts that are neither multiples of 4 nor equal, Cout across the 32-wide MFMA tile, the
pool, no CBN)."""
CASES = {
    "A": dict(cin=3, cout=10, bt=4, map=(5, 6), n_class=6, up=2, down=1, bn=True, seed=100),
    "B": dict(cin=12, cout=40, bt=3, map=(7, 5), n_class=6, up=2, down=1, bn=True, seed=200),
    "C": dict(cin=8, cout=8, bt=4, map=(5, 6), n_class=6, up=1, down=1, bn=True, seed=300),
    "D": dict(cin=3, cout=8, bt=4, map=(6, 6), n_class=6, up=1, down=2, bn=True, seed=400),
    "E": dict(cin=3, cout=10, bt=4, map=(5, 6), n_class=6, up=2, down=1, bn=False, seed=500),
}
