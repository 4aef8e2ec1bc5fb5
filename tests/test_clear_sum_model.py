"""The order k_shadow_clear adds a point's light samples in (rtx_shadow_clearlane.h clear_lane_sum) against the
order k_shadow does, as numpy float32 models, bit for bit.

k_shadow: lane l of the wave adds samples l, l + 64, l + 128, ... below nl to a sum that starts at +0, then
wave_sum adds lane ^ M's value to every lane for M = 32, 16, 8, 4, 2, 1; lane 0's total is the point's.

k_shadow_clear: the six-level nest, one lane doing it all.  Leaf t = 0 .. 63 is lane rev6(t) (0, 32, 16, 48,
...): its samples in index order from +0; the tree is folded as a binary counter, level b keeping the left
child until bit b of t brings the right one, the left operand the one with the lower lanes.
"""
import numpy as np
import pytest

f32 = np.float32
NLS = [64, 65, 127, 128, 300, 1023, 1025]


def terms(seed, nl):
    """nl triples of a wide exponent spread and both signs, some exact zeros of either sign"""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((nl, 3)) * np.exp2(rng.integers(-40, 40, (nl, 3)))).astype(f32)
    z = rng.random((nl, 3)) < 0.05
    c[z] = np.where(rng.random(int(z.sum())) < 0.5, f32(0.0), f32(-0.0))
    return c


def lanes_then_butterfly(c):
    nl = len(c)
    v = np.zeros((64, 3), f32)
    for base in range(0, nl, 64):
        pk = np.zeros((64, 3), f32)  # an idle lane adds +0
        n = min(64, nl - base)
        pk[:n] = c[base:base + n]
        v = (v + pk).astype(f32)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[lane ^ m]).astype(f32)
    return v[0]


def rev6(t):
    return int(format(t, "06b")[::-1], 2)


def nest(c):
    nl = len(c)
    s = [None] * 6
    x = None
    for t in range(64):
        x = np.zeros(3, f32)
        for idx in range(rev6(t), nl, 64):
            x = (x + c[idx]).astype(f32)
        for b in range(6):
            if not (t >> b) & 1:
                s[b] = x
                break
            x = (s[b] + x).astype(f32)
    return x


def test_the_leaf_order_is_the_bit_reversal():
    assert [rev6(t) for t in range(8)] == [0, 32, 16, 48, 8, 40, 24, 56]
    assert sorted(rev6(t) for t in range(64)) == list(range(64))


@pytest.mark.parametrize("nl", NLS)
def test_the_nest_gives_the_butterflys_bits(nl):
    differ = 0
    for seed in range(40):
        c = terms(1000 * nl + seed, nl)
        a, b = lanes_then_butterfly(c), nest(c)
        assert a.view(np.uint32).tolist() == b.view(np.uint32).tolist(), (nl, seed)
        # not vacuous: the plain index-order sum is another number
        plain = np.zeros(3, f32)
        for q in c:
            plain = (plain + q).astype(f32)
        differ += int((plain.view(np.uint32) != a.view(np.uint32)).any())
    assert differ > 20


def test_signed_zeros_and_short_lists():
    # every term -0: a lane's sum is +0 + -0 = +0, never -0, whatever the order
    for nl in (1, 63, 64, 65):
        c = np.full((nl, 3), -0.0, f32)
        a, b = lanes_then_butterfly(c), nest(c)
        assert a.view(np.uint32).tolist() == b.view(np.uint32).tolist() == [0, 0, 0]
