"""The host side of the synthetic-text generator (data/synth_text.py) and the numpy restatement of `mr_synth_render`
(tests/_synth_text_ref.py): planning is deterministic, the planned maps carry the quads to the line boxes, everything lies inside
its canvas, scene words do not overlap, labels are the charset's, and the restatement at the identity map returns the glyph boxes
byte for byte.  No GPU, and (but for the last test) no PIL: the atlases are random arrays."""
import numpy as np
import pytest

import _synth_text_ref as R
from megreader_amd.charsets import EnglishCharset
from megreader_amd.data import GlyphAtlas, SynthScenes, SynthStyle, SynthText
from megreader_amd.data.synth_text import CANVAS_DTYPE, ITEM_DTYPE, blur_taps, order_quad
from megreader_amd.structure.db_geometry import mini_box

WORDS = ["TEXT", "A", "MI355X", "GFX950", "READER", "0123456789"]


def random_atlas(charset, seed, gh=12):
    """Every alphanumeric class gets a glyph of 3..9 columns of random coverage; blank and unknown get none."""
    rng = np.random.RandomState(seed)
    w = np.zeros(len(charset), dtype=np.int32)
    w[2:] = rng.randint(3, 10, len(charset) - 2)
    x0 = np.concatenate([[0], np.cumsum(w)[:-1]]).astype(np.int32)
    return GlyphAtlas(rng.randint(0, 256, (gh, int(w.sum()))).astype(np.uint8), x0, w)


@pytest.fixture(scope="module")
def charset():
    return EnglishCharset()


@pytest.fixture(scope="module")
def atlases(charset):
    return [random_atlas(charset, 1, 12), random_atlas(charset, 2, 9)]


def carried(h9, pts):
    p = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(h9, dtype=np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:]


def check_plan(items, quads, atlases, H, W):
    assert len(items) == len(quads)
    for it, quad in zip(items, quads):
        atlas = atlases[int(it["font"])]
        lw = float(atlas.w[it["glyph"][:int(it["n_glyphs"])]].sum())
        want = np.array([[0.0, 0.0], [lw, 0.0], [lw, atlas.gh], [0.0, atlas.gh]])
        assert np.abs(carried(it["h"], quad) - want).max() < 1e-9
        assert (quad[:, 0] >= 0).all() and (quad[:, 0] <= W).all() and (quad[:, 1] >= 0).all() and (quad[:, 1] <= H).all()
        assert 0 <= it["x0"] < it["x1"] <= W and 0 <= it["y0"] < it["y1"] <= H
        assert it["x0"] <= np.floor(quad[:, 0].min()) and it["x1"] >= np.ceil(quad[:, 0].max())
        assert it["y0"] <= np.floor(quad[:, 1].min()) and it["y1"] >= np.ceil(quad[:, 1].max())


def test_struct_dtypes_mirror_the_header():
    assert ITEM_DTYPE.itemsize == 280 and CANVAS_DTYPE.itemsize == 88
    assert ITEM_DTYPE.fields["h"][1] == 80 and ITEM_DTYPE.fields["glyph"][1] == 152


def test_crop_plans_are_deterministic_per_seed_and_index(charset, atlases):
    a = SynthText(charset, atlases, WORDS, seed=5).plan(16, 3)
    b = SynthText(charset, atlases, WORDS, seed=5).plan(16, 3)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]
    c = SynthText(charset, atlases, WORDS, seed=5).plan(16, 4)
    d = SynthText(charset, atlases, WORDS, seed=6).plan(16, 3)
    assert a[0].tobytes() != c[0].tobytes() and a[0].tobytes() != d[0].tobytes()


@pytest.mark.parametrize("size", [(32, 128), (32, 100), (48, 64)])
def test_crop_plans_carry_quads_to_line_boxes_inside_the_canvas(charset, atlases, size):
    items, canvases, quads, texts = SynthText(charset, atlases, WORDS, image_size=size, seed=1).plan(64, 0)
    check_plan(items, quads, atlases, *size)
    assert (canvases["first_item"] == np.arange(64)).all() and (canvases["n_items"] == 1).all()
    assert (items["canvas"] == np.arange(64)).all()
    assert [len(t) for t in texts] == items["n_glyphs"].tolist()


def test_scene_plans_inside_the_canvas_without_overlap(charset, atlases):
    scenes = SynthScenes(charset, atlases, WORDS, canvas=(96, 160), words_per_scene=(2, 6), seed=2,
                         style=SynthStyle(scene_height=(0.1, 0.2)))
    total = 0
    for index in range(4):
        items, canvases, quads, texts, back = scenes.plan(3, index)
        assert back is None
        check_plan(items, quads, atlases, 96, 160)
        assert canvases["first_item"].tolist() == np.concatenate([[0], np.cumsum(canvases["n_items"])[:-1]]).tolist()
        for s in range(3):
            first, cnt = int(canvases["first_item"][s]), int(canvases["n_items"][s])
            assert cnt == len(texts[s]) <= 6 and (items["canvas"][first:first + cnt] == s).all()
            total += cnt
            box = [(q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()) for q in quads[first:first + cnt]]
            for i in range(cnt):
                for j in range(i):
                    a, b = box[i], box[j]
                    assert a[0] >= b[2] or a[2] <= b[0] or a[1] >= b[3] or a[3] <= b[1], (index, s, i, j)
    assert total >= 12                                     # words were placed
    again = scenes.plan(3, 1)
    assert again[0].tobytes() == scenes.plan(3, 1)[0].tobytes() != scenes.plan(3, 2)[0].tobytes()


def test_quads_are_ordered_as_the_representer_orders_boxes():
    rng = np.random.RandomState(3)
    for _ in range(20):
        a, b = rng.uniform(5, 40), rng.uniform(5, 40)
        t = rng.uniform(-0.7, 0.7)
        rect = np.array([[-a, -b], [a, -b], [a, b], [-a, b]]) @ np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]]) + 50
        want = np.array(mini_box(rect.tolist())[0])
        for shift in range(4):
            assert np.abs(order_quad(np.roll(rect, shift, axis=0)) - want).max() < 1e-9


def test_labels_are_the_charsets_encoding(charset, atlases):
    gen = SynthText(charset, atlases, ["abc", "MI355X", "z"], max_size=8)
    items, _, _, texts = gen.plan(12, 0)
    assert set(texts) == {"abc", "MI355X", "z"}
    for k, t in enumerate(texts):                          # the planned glyph ids are the labels `batch` uploads
        assert items["glyph"][k, :8].tolist() == charset.string_to_label(t, 8).tolist() and items["n_glyphs"][k] == len(t)
        assert not items["glyph"][k, 8:].any()


def test_undrawable_words_are_drawn_again_then_refused(charset, atlases):
    gen = SynthText(charset, atlases, ["OK", "no-glyph!", "X" * 40])
    assert set(gen.plan(20, 0)[3]) == {"OK"}
    with pytest.raises(ValueError):
        SynthText(charset, atlases, ["!!", ""]).plan(1, 0)
    calls = []
    SynthText(charset, atlases, lambda rng: calls.append(1) or "W%d" % rng.integers(10)).plan(5, 0)
    assert len(calls) == 5


def test_blur_taps_sum_to_one():
    for sigma in (0.3, 0.8, 2.0):
        w = blur_taps(sigma).astype(np.float64)
        assert w.dtype == np.float64 and abs(w[0] + 2 * w[1] + 2 * w[2] - 1.0) < 1e-6 and w[0] > w[1] > w[2] >= 0


def identity_tables(atlas, glyphs, H, W):
    items = np.zeros(1, dtype=ITEM_DTYPE)
    items["n_glyphs"][0] = len(glyphs)
    items["glyph"][0, :len(glyphs)] = glyphs
    items["h"][0] = np.eye(3).reshape(9)
    items["x1"], items["y1"] = W, H
    items["fg"] = 255.0
    canvases = np.zeros(1, dtype=CANVAS_DTYPE)
    canvases["n_items"] = 1
    return items, canvases


def test_restatement_at_identity_returns_the_glyph_boxes(charset, atlases):
    atlas = atlases[0]
    glyphs = [charset.index(ch) for ch in "GFX950"] + [0, 99]          # blank has no glyph, 99 is no class: both are skipped
    want = np.concatenate([atlas.coverage[:, atlas.x0[g]:atlas.x0[g] + atlas.w[g]] for g in glyphs[:6]], axis=1)
    H, W = atlas.gh + 3, want.shape[1] + 5
    items, canvases = identity_tables(atlas, glyphs, H, W)
    u8, f32 = R.render(canvases, items, [atlas], H, W, (1.0, 2.0, 3.0))
    assert u8.shape == (1, H, W, 3) and f32.shape == (1, 3, H, W) and u8.dtype == np.uint8 and f32.dtype == np.float32
    for c in range(3):
        assert np.array_equal(u8[0, :atlas.gh, :want.shape[1], c], want)
        assert not u8[0, atlas.gh:, :, c].any() and not u8[0, :, want.shape[1]:, c].any()
        assert np.array_equal(f32[0, c], ((u8[0, :, :, c].astype(np.float64) - (c + 1.0)).astype(np.float32) / np.float32(255)))


def test_from_font_on_pillows_own_font(charset, tmp_path):
    features = pytest.importorskip("PIL.features")
    if not features.check("freetype2"):
        pytest.skip("Pillow without FreeType: its built-in font has one small size")
    atlas = GlyphAtlas.from_font(charset, size=24)
    eligible = [i for i in range(len(charset)) if i not in (charset.blank, charset.unknown) and len(charset[i]) == 1]
    assert len(eligible) == 36 and (atlas.w[eligible] > 0).all()
    assert atlas.w[charset.blank] == 0 and atlas.w[charset.unknown] == 0
    assert atlas.w[charset.index("W")] > atlas.w[charset.index("I")]
    assert atlas.coverage.max() == 255 and atlas.coverage.shape[1] == int(atlas.w.sum())
    atlas.save(tmp_path / "atlas.npz")
    back = GlyphAtlas.load(tmp_path / "atlas.npz")
    assert np.array_equal(back.coverage, atlas.coverage) and np.array_equal(back.x0, atlas.x0) and np.array_equal(back.w, atlas.w)


def test_a_batch_of_homographies_equals_each_solved_alone():
    from megreader_amd.data.quad_crop import _homography, homographies
    rng = np.random.RandomState(4)
    src, dst = rng.uniform(0, 100, (9, 4, 2)), rng.uniform(0, 40, (9, 4, 2))
    got = homographies(src, dst)
    for k in range(9):
        assert got[k].tobytes() == _homography(src[k], dst[k]).tobytes()          # the planner's maps are the cropper's
        assert got[k][2, 2] == 1.0 and np.abs(carried(got[k], src[k]) - dst[k]).max() < 1e-9
