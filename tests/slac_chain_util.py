"""Shared by the GPU tests of the three SLAC latent chains (test_posterior_chain_gpu.py, test_latent_predict_gpu.py,
test_latent_imagine_gpu.py) and by tests/tools/bench_*: the C-ABI call counter and the seeded LatentModel."""
import torch

import slac_latent_ref as R


def count_calls(fn):
    """C-ABI calls per entry point during fn().  Every one of these entry points is one launch at the sizes of the tests, except
    s2p_linear_add_bwd / s2p_linear_bwd with both a weight gradient and a dgrad: two."""
    from s2p_amd import _lib
    L, counts, orig = _lib.lib(), {}, {}
    for name in _lib.SIGNATURES:
        f = getattr(L, name)
        orig[name] = f

        def wrap(*a, _f=f, _n=name):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a)
        setattr(L, name, wrap)
    try:
        fn()
    finally:
        for name, f in orig.items():
            setattr(L, name, f)
    return counts


def build_model(A, dtype=torch.float32):
    """A LatentModel of action width A with the seeded weights of tests/slac_latent_ref.py."""
    from s2p_amd.slac import LatentModel
    m = LatentModel((3, 100, 100), (A,), image_size=100, dtype=dtype)
    m.load_state_dict(R.full_state_dict(R.make_params(A)), strict=True)
    return m


def model_cache():
    """action width -> build_model(A), built once: the body of each test file's module-scoped `models` fixture."""
    cache = {}

    def get(A):
        if A not in cache:
            cache[A] = build_model(A)
        return cache[A]
    return get
