"""ba_amd/scene.py: the generator draws the same scene however it is computed.  Candidate poses
come from the head of a random order per row (random_order_head, the former
np.argsort(rng.random(...))[:, :k]); chunks of landmarks are generated on threads."""
import numpy as np
import pytest

from ba_amd import scene


class _Coarse:
    """A stream of uniforms rounded to 1/levels: many ties, drawn row-major like Generator.random."""

    def __init__(self, seed, levels):
        self.g, self.levels = np.random.default_rng(seed), levels

    def random(self, shape):
        return np.floor(self.g.random(shape) * self.levels) / self.levels


@pytest.mark.parametrize("m,ncol,k,levels", [(1000, 2500, 48, None), (3000, 200, 12, None), (500, 96, 48, None),
                                              (700, 300, 20, 40), (700, 300, 20, 4000), (50, 48, 48, None)])
def test_random_order_head_is_the_argsort_head(m, ncol, k, levels):
    mk = (lambda: np.random.default_rng(5)) if levels is None else (lambda: _Coarse(5, levels))
    ref = np.argsort(mk().random((m, ncol)), axis=1)[:, :k]
    got = scene.random_order_head(mk(), m, ncol, k, block=128)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)


def test_scene_does_not_depend_on_the_thread_count():
    kw = dict(lm_dim=1, seed=9, chunk=1500)
    a = scene.make_scene(800, 6000, 8, threads=1, **kw)
    b = scene.make_scene(800, 6000, 8, threads=4, **kw)
    for name, v in vars(a).items():
        if isinstance(v, np.ndarray):
            assert v.dtype == getattr(b, name).dtype and np.array_equal(v, getattr(b, name)), name
