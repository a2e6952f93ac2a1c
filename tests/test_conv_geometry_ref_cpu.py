"""What can be settled without a GPU about the exact convolution cases of tests/_conv_geometry_ref.py: the integer operands
keep every bf16 result an integer bf16 holds, the float64 reference is told apart from two deliberately wrong gathers on every
padded side of every case, the named edge geometries have the property they are named after, the reference does not rest on
one library call, and the kernel x geometry lists name only cases the kernels serve."""
import collections

import pytest
import torch

import _conv_geometry_ref as R


def _fwd_keys():
    return sorted({(gid, cg, R.out_channels(gid, cg), R.NT_KERNELS[k][0]) for k, gid, cg in R.nt_cases(False)})


def _dgrad_keys():
    keys = {(gid, R.out_channels(gid, cg), cg, R.NT_KERNELS[k][0]) for k, gid, cg in R.nt_cases(True)}
    keys |= {(gid, R.out_channels(gid, cg), cg, R.BF16) for gid, cg in R.dgrad_add_cases()}
    return sorted(keys)


def _id(key):
    return "%s-c%d-k%d-%s" % key


def test_geometry_table():
    sizes = {gid: R.out_size(g) for gid, g in R.GEOMETRIES.items()}
    print(sizes)
    assert sizes["k3_p1"] == (5, 7) and R.GEOMETRIES["k3_p1"].N * 35 == 280      # one 256- / 272-row tile + an edge tile
    assert sizes["k2_p0_ho1"][0] == 1 and sizes["k3_1x1img"] == (1, 1) and sizes["k7_s2_p3"] == (6, 7)
    assert R.taps(R.GEOMETRIES["k48_32taps"]) == 32 and R.taps(R.GEOMETRIES["k3x11_33taps"]) == 33
    assert R.taps(R.GEOMETRIES["k5_p2"]) == 25 and R.taps(R.GEOMETRIES["k7_s2_p3"]) == 49
    assert all(h >= 1 and w >= 1 for h, w in sizes.values())
    for gid in R.GEOMETRIES:
        assert R.gathered_channels(gid, R.F32) == (32, 64, 4)
        bf = R.gathered_channels(gid, R.BF16)
        assert {8, 24} <= set(bf) and all(R.taps(R.GEOMETRIES[gid]) * c <= 2112 for c in bf)
        assert (128 in bf) == (R.taps(R.GEOMETRIES[gid]) <= 9)
    assert R.padded_ld(72) == 80 and R.padded_ld(64) == 72 and R.padded_ld(44) == 56


def test_case_lists_name_only_what_the_kernels_serve():
    for dgrad in (False, True):
        cases = R.nt_cases(dgrad)
        assert len(set(cases)) == len(cases)
        per_kernel = collections.Counter(k for k, _, _ in cases)
        print("dgrad" if dgrad else "forward", len(cases), dict(per_kernel))
        assert set(per_kernel) == set(R.NT_KERNELS)                       # no kernel without a case
        for kernel, gid, cg in cases:
            g, dtype = R.GEOMETRIES[gid], R.NT_KERNELS[kernel][0]
            assert cg % R.VEC[dtype] == 0 and cg in R.gathered_channels(gid, dtype)
            if kernel in R.WIDE_KERNELS:
                assert dtype == R.BF16 and cg % 64 == 0 and R.taps(g) <= 32 and not (dgrad and (g.sh, g.sw) != (1, 1))
            if kernel == "ksplit4":
                assert cg == 128 and (g.R, g.S) == (3, 3)
        for kernel in ("default", "default_f32", "tile128_2buf", "tile64_4buf", "tile96x64", "staged", "tile128_f32", "tile64_f32",
                       "staged_f32"):
            assert {gid for k, gid, _ in cases if k == kernel} == set(R.GEOMETRIES), kernel
        # every kind of output width, ReLU on and off, on every kernel that has more than a handful of cases
        for kernel in R.NT_KERNELS:
            mine = [(gid, cg) for k, gid, cg in cases if k == kernel]
            if len(mine) >= 8:
                assert {R.out_channels(gid, cg) for gid, cg in mine} == set(R.OUT_CHANNELS), kernel
                assert {R.relu_of(gid, cg) for gid, cg in mine} == {0, 1}, kernel
    assert [gid for gid, _ in R.dgrad_add_cases()] == list(R.GEOMETRIES)
    wg = R.wgrad_cases()
    assert len(set(wg)) == len(wg)
    print("wgrad", len(wg), dict(collections.Counter(v for v, _, _, _ in wg)))
    for variant, gid, cin, cout in wg:
        g = R.GEOMETRIES[gid]
        assert variant != "tab" or R.taps(g) <= 32
        assert cout in R.OUT_CHANNELS and cin in R.gathered_channels(gid, R.wgrad_dtype(variant))
        if variant == "taps":
            assert ((g.R, g.S, g.sh, g.sw) == (3, 3, 1, 1) and g.ph == g.dh == g.pw == g.dw and cin % 64 == 0
                    and cout % 8 == 0 and (g.H * (g.W + g.dh) + 7) // 8 * 8 >= 32)
    assert collections.Counter(v for v, _, _, _ in wg)["taps"] == 4
    assert {v for v, _, _, _ in wg} == {"wgrad_bf16", "wgrad_f32", "tab", "taps"}


def _differs_on_every_side(c, wrong, name):
    """y on the output rows / columns whose windows reach into a padded side; for the replicated border also dx on the input
    border row / column beside that side, where the gradient of the padding lands (a stride may leave that row untouched by the
    true gather, so the rotated kernel is only required to change dx somewhere)."""
    g = c.geom
    y_w, dx_w = wrong
    border = {"top": (1, 0), "bottom": (1, g.H - 1), "left": (2, 0), "right": (2, g.W - 1)}
    for side, (idx, axis) in R.padded_sides(g).items():
        sel = torch.tensor(idx)
        assert not torch.equal(c.y.index_select(axis, sel), y_w.index_select(axis, sel)), (name, side, "y")
        ax, at = border[side]
        if name == "replicate":
            assert not torch.equal(c.dx.select(ax, at), dx_w.select(ax, at)), (name, side, "dx")


@pytest.mark.parametrize("key", _fwd_keys(), ids=_id)
def test_forward_case_is_exact_and_discriminates(key):
    gid, cin, cout, dtype = key
    c = R.conv_case(gid, cin, cout)
    g = c.geom
    assert c.y.shape == (g.N,) + R.out_size(g) + (cout,) and torch.equal(c.y, c.y.round())
    assert int(c.x.abs().max()) == 2 and int(c.w_krsc.abs().max()) == 1 and int(c.bias.abs().max()) <= 4
    peak = float(c.y.abs().max())
    print("%s: K = %d, max |y| = %g" % (_id(key), R.taps(g) * cin, peak))
    if dtype == R.BF16:
        assert peak <= R.BF16_EXACT
        assert torch.equal(R.to_dtype(c.y, dtype).double(), c.y)
    assert float(torch.relu(c.y).sum()) > 0 and float(torch.relu(-c.y).sum()) > 0      # the ReLU cases clamp something
    wrong = R.wrong_references(c)
    if g.ph or g.pw:
        assert R.padded_sides(g), "a padded geometry whose padding no window reaches"
        _differs_on_every_side(c, wrong["replicate"], "replicate")
    else:
        assert torch.equal(wrong["replicate"][0], c.y)
    if R.taps(g) > 1 and (g.H, g.W) != (1, 1):
        # (on the 1x1 image the only tap inside the image is the centre one, which the rotation fixes: the replicated border,
        # which makes all nine taps valid, is what tells a wrong mask apart there)
        assert not torch.equal(wrong["rot180"][0], c.y) and not torch.equal(wrong["rot180"][1], c.dx)
        _differs_on_every_side(c, wrong["rot180"], "rot180")


@pytest.mark.parametrize("key", _dgrad_keys(), ids=_id)
def test_dgrad_case_is_exact_and_discriminates(key):
    gid, cin, cout, dtype = key               # cout = the gathered channel count of the dgrad
    c = R.conv_case(gid, cin, cout)
    g = c.geom
    assert c.dx.shape == (g.N, g.H, g.W, cin) and torch.equal(c.dx, c.dx.round())
    peak = float(c.dx.abs().max())
    print("%s: K = %d, max |dx| = %g" % (_id(key), R.taps(g) * cout, peak))
    if dtype == R.BF16:
        assert peak <= R.BF16_EXACT
        if (gid, cout) in R.dgrad_add_cases():
            assert float((c.dx + R.addend_for(c)).abs().max()) <= R.BF16_EXACT
    wrong = R.wrong_references(c)
    if g.ph or g.pw:
        _differs_on_every_side(c, wrong["replicate"], "replicate")
    if R.taps(g) > 1 and (g.H, g.W) != (1, 1):
        _differs_on_every_side(c, wrong["rot180"], "rot180")
        assert not torch.equal(wrong["rot180"][1], c.dx)


def test_windows_wholly_in_padding_give_the_bias():
    for cin in R.gathered_channels("k3_p3_overpad", R.BF16):
        c = R.conv_case("k3_p3_overpad", cin, R.out_channels("k3_p3_overpad", cin))
        for h in (0, -1):
            for w in (0, -1):
                assert torch.equal(torch.relu(c.y[:, h, w]), torch.relu(c.bias).expand(c.geom.N, -1))
        assert not torch.equal(c.y[:, 1, 1], c.bias.expand(c.geom.N, -1))
    # padding 2 under a 3x3 kernel: the corner window still holds the image's corner pixel under its last tap, nothing else
    for cin in R.gathered_channels("k3_p2_overpad", R.BF16):
        c = R.conv_case("k3_p2_overpad", cin, R.out_channels("k3_p2_overpad", cin))
        one_tap = torch.einsum("nc,kc->nk", c.x[:, 0, 0], c.w_krsc[:, 2, 2]) + c.bias
        assert torch.equal(c.y[:, 0, 0], one_tap) and not torch.equal(c.y[:, 0, 0], c.bias.expand(c.geom.N, -1))


def test_strided_dgrad_leaves_the_untouched_row_zero():
    g = R.GEOMETRIES["k3_s2_p0_untouched"]
    for dtype in (R.BF16, R.F32):
        for cg in R.gathered_channels(g.id, dtype):
            c = R.conv_case(g.id, R.out_channels(g.id, cg), cg)
            assert c.dx.shape[1] == 10 and not c.dx[:, 9].any() and not c.dx[:, :, 7].any()
            assert all(bool(c.dx[:, h].any()) for h in range(9))


@pytest.mark.parametrize("gid", ["k3_1x1img", "k2_p0_ho1", "k3_p2_overpad"])
def test_reference_agrees_with_seven_plain_loops(gid):
    c = R.conv_case(gid, 4, 44, batch=8)
    y, dx = R.seven_loops(c)
    assert torch.equal(y + c.bias, c.y) and torch.equal(dx, c.dx)
    assert y.abs().sum() > 0 and dx.abs().sum() > 0
