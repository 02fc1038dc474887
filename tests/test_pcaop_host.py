"""Host: the fixed-point model of the PCA operator halves (tests/pcaop_ref.py) against its exact route, on the inputs
tests/test_gpu_pcaop.py gives the device.  The model meets the derived bounds; a model with one digit fewer, or with one
exponent for the whole block, leaves them -- so a device that did either would fail the GPU test."""
import numpy as np
import pytest

from tests import pcaop_ref as ref

_PANELS = {}


def _panel(shape):
    if shape not in _PANELS:
        n, m = shape
        G, _ = ref.panel(31 + n, n, m)
        _PANELS[shape] = (G,) + ref.center_scale(G)
    return _PANELS[shape]


def _cases():
    # every shape with a wide and a narrow block, every block width on the shape with two chunks on both sides, and the
    # special operands on the smallest and on the largest shape
    out = [(s, b, "normal") for s in ref.SHAPES for b in (5, 64)]
    out += [((129, 257), b, "normal") for b in ref.BS if b not in (5, 64)]
    out += [(s, 6, kind) for s in ((33, 130), (200, 1000)) for kind in ref.KINDS[1:]]
    return out


CASES = _cases()


@pytest.mark.parametrize("shape,b,kind", CASES)
def test_model_meets_its_bounds(shape, b, kind):
    G, center, scale = _panel(shape)
    n, m = G.shape
    Q = ref.operand(kind, n, b, 7)
    W = ref.model_zt(G, center, scale, Q)
    ezt = np.abs(W - ref.exact_zt(G, center, scale, Q))
    bzt = ref.bound_zt(G, center, scale, Q)
    assert np.all(ezt <= bzt), (ezt / bzt).max()
    Win = ref.operand(kind, m, b, 8)
    Y = ref.model_z(G, center, scale, Win)
    ez = np.abs(Y - ref.exact_z(G, center, scale, Win))
    bz = ref.bound_z(G, center, scale, Win)
    assert np.all(ez <= bz), (ez / bz).max()
    if kind == "zero_col":  # exact zeros, and no bound to speak of
        assert np.all(W[:, b // 2] == 0) and np.all(Y[:, b // 2] == 0)
        assert np.all(bzt[:, b // 2] == 0) and np.all(bz[:, b // 2] == 0)
    # the composition against numpy's FP64, as the GPU test takes it
    Z = ref.scaled(G, center, scale)
    comp = np.abs(ref.model_z(G, center, scale, W) - Z @ (Z.T @ Q))
    assert np.all(comp <= ref.bound_apply(G, center, scale, Q, W))


def test_exact_route_agrees_with_long_double():
    # the exact route is integer arithmetic; a long-double product of the same inputs is within ITS rounding of it
    G, center, scale = _panel((129, 257))
    n, m = G.shape
    Q = ref.operand("normal", n, 5, 3)
    LD = np.longdouble
    Z = (G.astype(LD) - center.astype(LD)[None, :]) / scale.astype(LD)[None, :]
    want = Z.T @ Q.astype(LD)
    mag = np.abs(Z).T @ np.abs(Q).astype(LD)
    assert np.all(np.abs(ref.exact_zt(G, center, scale, Q).astype(LD) - want) <= (n + 4) * 2.0 ** -63 * mag + 2.0 ** -53 * np.abs(want))
    Win = ref.operand("normal", m, 5, 4)
    Wp = (Win / scale[:, None]).astype(LD)
    Gc = G.astype(LD) - center.astype(LD)[None, :]
    want = Gc @ Wp
    mag = np.abs(Gc) @ np.abs(Wp)
    assert np.all(np.abs(ref.exact_z(G, center, scale, Win).astype(LD) - want) <= (m + 4) * 2.0 ** -63 * mag + 2.0 ** -53 * np.abs(want))


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_bounds_have_teeth_one_digit_fewer(shape):
    G, center, scale = _panel(shape)
    n, m = G.shape
    Q = ref.operand("normal", n, 5, 7)
    ezt = np.abs(ref.model_zt(G, center, scale, Q, tu=ref.TU - 1) - ref.exact_zt(G, center, scale, Q))
    assert np.any(ezt > ref.bound_zt(G, center, scale, Q))
    Win = ref.operand("normal", m, 5, 8)
    ez = np.abs(ref.model_z(G, center, scale, Win, tu=ref.TU - 1) - ref.exact_z(G, center, scale, Win))
    assert np.any(ez > ref.bound_z(G, center, scale, Win))


@pytest.mark.parametrize("shape", ((33, 130), (200, 1000)))
def test_bounds_have_teeth_one_exponent_for_the_block(shape):
    G, center, scale = _panel(shape)
    n, m = G.shape
    Q = ref.operand("two_mag", n, 6, 7)
    ezt = np.abs(ref.model_zt(G, center, scale, Q, per_column=False) - ref.exact_zt(G, center, scale, Q))
    bzt = ref.bound_zt(G, center, scale, Q)
    assert np.all(ezt[:, 0::2] <= bzt[:, 0::2])  # the strong columns keep their exponent ...
    assert np.any(ezt[:, 1::2] > bzt[:, 1::2])   # ... the weak ones lose 23 bits
    Win = ref.operand("two_mag", m, 6, 8)
    ez = np.abs(ref.model_z(G, center, scale, Win, per_column=False) - ref.exact_z(G, center, scale, Win))
    assert np.any(ez[:, 1::2] > ref.bound_z(G, center, scale, Win)[:, 1::2])


def test_digits_are_balanced_and_recombine():
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((300, 4)) * np.array([1.0, 1e-7, 3e5, 2.0 ** -30]))
    X[0, 0] = -np.abs(X[:, 0]).max() * (1 - 2.0 ** -50)  # next to the top of the range
    amax, FU = ref.exponents(X)
    Wi = ref.fixed(X, FU)
    assert np.all(np.abs(Wi) <= 2 ** (7 * ref.TU - 2))
    d = ref.digits(Wi)
    assert d.min() >= -64 and d.max() <= 63
    assert np.array_equal(sum(d[t] * 128 ** t for t in range(ref.TU)), Wi)
    assert np.all(np.abs(np.ldexp(Wi.astype(float), (-FU[None, :]).astype(np.int32)) - X) <= 2.0 ** -40 * amax[None, :])
