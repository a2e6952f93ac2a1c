"""Synthetic text on the GPU: labelled word crops for the recognisers and labelled scenes for the DB detector and `TextReader`,
rendered where they are consumed.

The recognition configurations train on Synth90k and SynthText -- rendered text -- which nobody who checks this project out
has.  Here the host only PLANS: which word, which font, where its four corners lie on the canvas, colours, shadow, blur and noise,
all in float64 from `numpy.random.Generator([seed, batch index])`; `mr_synth_render` (csrc/synth_text.hip, the rule is written out
in include/megreader_hip.h) draws every canvas of the batch in ONE launch from glyph atlases that stay on the device.

    atlas = GlyphAtlas.from_font(charset)                       # host, PIL; or GlyphAtlas(coverage, x0, w) from arrays
    crops = SynthText(charset, [atlas], ['hello', 'world'], image_size=(32, 128), seed=0)
    batch = crops.batch(256)              # {'image' f32 [256, 3, 32, 128], 'label' i32 [256, 32], 'length' i32 [256], 'text'}
    scenes = SynthScenes(charset, [atlas], words, canvas=(640, 640), words_per_scene=(1, 12))
    batch = scenes.batch(8)               # {'photos' u8 [8, 640, 640, 3], 'polygons', 'ignore_tags', 'texts'}

Coordinates.  Canvas and line coordinates are continuous with pixel k covering [k, k + 1): a word's virtual line image (its
glyphs' advance boxes side by side, Lw x gh) has the corners (0, 0), (Lw, 0), (Lw, gh), (0, gh); the planner chooses the four
canvas points they land on and solves the projective map canvas -> line through them (`homographies` of data/quad_crop.py).  The
ground-truth quadrilateral is those four canvas points, ordered as `SegDetectorRepresenter` orders its boxes.
"""
import ctypes

import numpy as np
import torch

from .._lib import STRUCTS, _DEFINES, call, load, ptr
from ..charsets import EnglishCharset
from .device_pipeline import RGB_MEAN
from .quad_crop import homographies
from .staging import Sections, Staging, upload

MAX_GLYPHS = _DEFINES["MR_SYNTH_MAX_GLYPHS"]
MAX_ITEMS = _DEFINES["MR_SYNTH_MAX_ITEMS"]
MAX_GLYPH_W = _DEFINES["MR_SYNTH_MAX_GLYPH_W"]


class SynthFont(ctypes.Structure):
    """struct mr_synth_font of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_synth_font"]


class SynthItem(ctypes.Structure):
    """struct mr_synth_item of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_synth_item"]


class SynthCanvas(ctypes.Structure):
    """struct mr_synth_canvas of include/megreader_hip.h."""
    _fields_ = STRUCTS["mr_synth_canvas"]


FONT_DTYPE = np.dtype(SynthFont)
ITEM_DTYPE = np.dtype(SynthItem)
CANVAS_DTYPE = np.dtype(SynthCanvas)


class GlyphAtlas(object):
    """One font: `coverage` uint8 [gh, aw], and per class id `x0` (the glyph's first column) and `w` (its advance box; 0: the
    class has no glyph)."""

    def __init__(self, coverage, x0, w):
        self.coverage = np.ascontiguousarray(coverage, dtype=np.uint8)
        self.x0 = np.ascontiguousarray(x0, dtype=np.int32)
        self.w = np.ascontiguousarray(w, dtype=np.int32)
        if self.coverage.ndim != 2 or self.coverage.shape[0] < 1 or self.coverage.shape[1] < 1:
            raise ValueError("GlyphAtlas: coverage must be uint8 [gh, aw], got shape %s" % (self.coverage.shape,))
        if self.x0.ndim != 1 or self.x0.shape != self.w.shape:
            raise ValueError("GlyphAtlas: x0 and w are one int per class, got %s and %s" % (self.x0.shape, self.w.shape))
        bad = (self.w != 0) & ((self.w < 0) | (self.w > MAX_GLYPH_W) | (self.x0 < 0)
                               | (self.x0.astype(np.int64) + self.w > self.coverage.shape[1]))
        if bad.any():
            raise ValueError("GlyphAtlas: the boxes of classes %s do not lie inside the atlas" % np.nonzero(bad)[0].tolist())

    @property
    def gh(self):
        return int(self.coverage.shape[0])

    @property
    def n_classes(self):
        return int(self.w.shape[0])

    def has_glyph(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        ok = (ids >= 0) & (ids < self.n_classes)
        return ok & (self.w[np.where(ok, ids, 0)] > 0)

    @classmethod
    def from_font(cls, charset, font=None, size=48):
        """Render one glyph per class of `charset` that is a single character, neither blank nor unknown -- the class's own
        character, whatever case the charset folds queries to.  font: None (Pillow's built-in font), a path, or an `ImageFont`."""
        from PIL import Image, ImageDraw, ImageFont
        if font is None:
            try:
                font = ImageFont.load_default(size=size)
            except TypeError:                               # a Pillow whose built-in font has one size
                font = ImageFont.load_default()
        elif isinstance(font, (str, bytes)) or hasattr(font, "__fspath__"):
            font = ImageFont.truetype(font, size)
        chars = {}
        for i in range(len(charset)):
            ch = charset[i]
            if isinstance(ch, str) and len(ch) == 1 and i not in (charset.blank, charset.unknown):
                chars[i] = ch
        boxes = {i: font.getbbox(ch) for i, ch in chars.items()}            # (left, top, right, bottom) from the origin
        if not boxes:
            raise ValueError("GlyphAtlas.from_font: the charset has no single-character class")
        top = min(b[1] for b in boxes.values())
        gh = max(max(b[3] for b in boxes.values()) - top, 1)
        x0 = np.zeros(len(charset), dtype=np.int32)
        w = np.zeros(len(charset), dtype=np.int32)
        tiles, at = [], 0
        for i, ch in chars.items():
            left, _, right, _ = boxes[i]
            lead = max(-int(np.floor(left)), 0)                                 # bearings go inside the box
            width = max(int(np.ceil(font.getlength(ch))), int(np.ceil(right))) + lead
            if width < 1:
                continue
            tile = Image.new("L", (width, gh), 0)
            ImageDraw.Draw(tile).text((lead, -top), ch, fill=255, font=font)
            tiles.append(np.asarray(tile, dtype=np.uint8))
            x0[i], w[i] = at, width
            at += width
        return cls(np.concatenate(tiles, axis=1), x0, w)

    def save(self, path):
        np.savez_compressed(path, coverage=self.coverage, x0=self.x0, w=self.w)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["coverage"], z["x0"], z["w"])


class SynthStyle(object):
    """The ranges the planner draws from (uniformly unless said otherwise).  The defaults give legible crops."""

    def __init__(self, height=(0.6, 0.9), width=(0.85, 0.98), scene_height=(0.04, 0.1), rotation=(-4.0, 4.0),
                 shear=(-0.15, 0.15), perspective=0.06, min_contrast=80.0, gradient=(0.0, 40.0), shadow_prob=0.3,
                 shadow_offset=(0.5, 3.0), shadow_alpha=(0.3, 0.8), blur_sigma=(0.0, 0.9), noise=(0.0, 12.0)):
        self.height = height                    # text height over the canvas height (word crops)
        self.width = width                      # text width over the canvas width (word crops: the word fills the crop)
        self.scene_height = scene_height        # text height over the canvas height (scenes; the aspect is the font's)
        self.rotation = rotation                # degrees
        self.shear = shear                      # x += shear * y
        self.perspective = perspective          # each corner moves by up to this fraction of the text height
        self.min_contrast = min_contrast        # |luma(fg) - luma(bg)|, 0..255
        self.gradient = gradient                # largest channel difference between the background's two colours
        self.shadow_prob = shadow_prob
        self.shadow_offset = shadow_offset      # line pixels, either sign
        self.shadow_alpha = shadow_alpha
        self.blur_sigma = blur_sigma            # canvas pixels; below 0.1 the blur is off
        self.noise = noise                      # amplitude: the noise is uniform in [-amp / 2, amp / 2)


def blur_taps(sigma):
    """(w0, w1, w2) of the 5-tap Gaussian of `sigma` (a number, or an array: then [n, 3]), normalised to sum 1 in float64, as
    float32."""
    sigma = np.asarray(sigma, dtype=np.float64)
    d = np.exp(-np.arange(3, dtype=np.float64) ** 2 / (2.0 * sigma[..., None] ** 2))
    return (d / (d[..., 0:1] + 2.0 * d[..., 1:2] + 2.0 * d[..., 2:3])).astype(np.float32)


def luma(bgr):
    bgr = np.asarray(bgr, dtype=np.float64)
    return 0.114 * bgr[..., 0] + 0.587 * bgr[..., 1] + 0.299 * bgr[..., 2]


def order_quad(quad):
    """The four corners in `SegDetectorRepresenter`'s order (structure/db_geometry.py `mini_box`): sorted by x; of the two
    left-most the upper one first and the lower one last, of the two right-most the upper one second."""
    p = sorted(np.asarray(quad, dtype=np.float64).reshape(4, 2).tolist(), key=lambda c: c[0])
    i1, i4 = (0, 1) if p[1][1] > p[0][1] else (1, 0)
    i2, i3 = (2, 3) if p[3][1] > p[2][1] else (3, 2)
    return np.array([p[i1], p[i2], p[i3], p[i4]], dtype=np.float64)


def word_quads(rng, style, cx, cy, half_w, half_h, H, W):
    """Quadrilaterals [n, 4, 2] (TL, TR, BR, BL of the line box): rectangles of the given centres and half sizes, sheared,
    rotated, their corners jittered, then shrunk about their bounding box's centre and shifted until they lie inside the canvas."""
    n = len(cx)
    base = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
    x = base[None, :, 0] * half_w[:, None]
    y = base[None, :, 1] * half_h[:, None]
    x = x + rng.uniform(style.shear[0], style.shear[1], n)[:, None] * y
    th = np.deg2rad(rng.uniform(style.rotation[0], style.rotation[1], n))[:, None]
    q = np.stack([np.cos(th) * x - np.sin(th) * y, np.sin(th) * x + np.cos(th) * y], axis=-1)
    q = q + rng.uniform(-1.0, 1.0, (n, 4, 2)) * (style.perspective * 2.0 * half_h)[:, None, None]
    lo, hi = q.min(axis=1), q.max(axis=1)
    size = np.maximum(hi - lo, 1e-9)
    room = np.array([W - 1.0, H - 1.0])
    s = np.minimum(1.0, (room / size).min(axis=1))
    q = (q - ((lo + hi) / 2.0)[:, None, :]) * s[:, None, None]
    half = size * s[:, None] / 2.0
    centre = np.clip(np.stack([cx, cy], axis=-1), 0.5 + half, np.array([W, H]) - 0.5 - half)
    return q + centre[:, None, :]


def contrasting(rng, style, bg):
    """A colour per row of bg [n, 3] whose luma differs from bg's by at least style.min_contrast: the first of 8 uniform draws
    that does, else black or white, whichever is farther."""
    n = len(bg)
    cand = rng.uniform(0.0, 255.0, (n, 8, 3))
    ok = np.abs(luma(cand) - luma(bg)[:, None]) >= style.min_contrast
    first = ok.argmax(axis=1)
    col = cand[np.arange(n), first]
    none = ~ok.any(axis=1)
    col[none] = np.where(luma(bg[none])[:, None] >= 127.5, 0.0, 255.0)
    return col


def fill_items(items, rng, style, canvas, font, glyphs, counts, lw, gh, quads, H, W):
    """Fill the ITEM_DTYPE array `items` for words of glyph ids glyphs[k, :counts[k]] on font[k], whose line boxes of lw[k] x gh[k]
    land on quads[k]; the colours are the caller's.  Draws the shadows from rng.  No loop over the items."""
    n = len(items)
    items["canvas"], items["font"], items["n_glyphs"], items["glyph"] = canvas, font, counts, glyphs
    shadow_on = rng.uniform(0.0, 1.0, n) < style.shadow_prob
    mag = rng.uniform(style.shadow_offset[0], style.shadow_offset[1], (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    items["shadow_dx"], items["shadow_dy"] = mag[:, 0], mag[:, 1]
    items["shadow_alpha"] = np.where(shadow_on, rng.uniform(style.shadow_alpha[0], style.shadow_alpha[1], n), 0.0)
    if n == 0:
        return items
    zero = np.zeros(n)
    line = np.stack([np.stack([zero, zero], -1), np.stack([lw, zero], -1), np.stack([lw, gh], -1), np.stack([zero, gh], -1)], 1)
    h = homographies(quads, line)
    items["h"] = h.reshape(n, 9)
    # the box: the line box grown by the taps' reach and the shadow's offset, carried back to the canvas
    m = 1.5 + np.abs(mag).max(axis=1)
    grown = np.stack([np.stack([-m, -m], -1), np.stack([lw + m, -m], -1), np.stack([lw + m, gh + m], -1),
                      np.stack([-m, gh + m], -1)], 1)
    back = np.concatenate([grown, np.ones((n, 4, 1))], axis=2) @ np.linalg.inv(h).transpose(0, 2, 1)
    front = (back[:, :, 2] > 0).all(axis=1)                     # else the grown box crosses the map's horizon: the whole canvas
    pts = back[:, :, :2] / np.where(front[:, None, None], back[:, :, 2:], 1.0)
    lo = np.floor(np.minimum(pts.min(axis=1), quads.min(axis=1))) - 1
    hi = np.ceil(np.maximum(pts.max(axis=1), quads.max(axis=1))) + 1
    lo = np.where(front[:, None], np.maximum(lo, 0.0), 0.0)
    hi = np.where(front[:, None], np.minimum(hi, [W, H]), [W, H])
    items["x0"], items["y0"], items["x1"], items["y1"] = lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1]
    return items


def fill_canvases(canvases, rng, style, H, W):
    """Background colours and gradient, blur taps, noise and seed of every canvas; first_item / n_items are the caller's."""
    n = len(canvases)
    bg0 = rng.uniform(0.0, 255.0, (n, 3))
    delta = rng.uniform(-1.0, 1.0, (n, 3)) * rng.uniform(style.gradient[0], style.gradient[1], n)[:, None]
    bg1 = np.clip(bg0 + delta, 0.0, 255.0)
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    span = np.abs(np.cos(th)) * W + np.abs(np.sin(th)) * H          # t runs over [0, 1] across the canvas
    gx, gy = np.cos(th) / span, np.sin(th) / span
    g0 = -(np.minimum(gx, 0.0) * W + np.minimum(gy, 0.0) * H)
    canvases["bg0"], canvases["bg1"] = bg0, bg1
    canvases["gx"], canvases["gy"], canvases["g0"] = gx, gy, g0
    sigma = rng.uniform(style.blur_sigma[0], style.blur_sigma[1], n)
    on = sigma >= 0.1
    taps = np.where(on[:, None], blur_taps(np.where(on, sigma, 1.0)), 0.0)
    canvases["blur"], canvases["w0"], canvases["w1"], canvases["w2"] = on, taps[:, 0], taps[:, 1], taps[:, 2]
    canvases["noise_amp"] = rng.uniform(style.noise[0], style.noise[1], n)
    canvases["seed"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return bg0, bg1


def shadow_colours(items, fg, ground):
    """The items' foreground colours, and their shadows: black on a ground light enough to show it, else white."""
    items["fg"] = fg
    items["shadow"] = np.where((luma(ground) >= 100.0)[:, None], 0.0, 255.0)


class SynthRenderer(object):
    """The device side: the atlases, their glyph pairs and the font table stay resident in one buffer; `render` stages the item
    and canvas tables (and whatever else the caller appends) in one pinned copy and makes the one launch."""

    def __init__(self, atlases, device=None):
        self.atlases = list(atlases)
        if not self.atlases:
            raise ValueError("synthetic text needs at least one GlyphAtlas")
        self.device = torch.device(device if device is not None else "cuda")
        load()
        fonts = np.zeros(len(self.atlases), dtype=FONT_DTYPE)
        pairs = np.concatenate([np.stack([a.x0, a.w], axis=1) for a in self.atlases]).astype(np.int32)
        lay = Sections([a.coverage for a in self.atlases] + [pairs, fonts], pad_end=True)
        first = 0
        for f, (a, off) in enumerate(zip(self.atlases, lay.offsets)):
            fonts["atlas_off"][f], fonts["pitch"][f] = off, a.coverage.shape[1]
            fonts["gh"][f], fonts["aw"][f] = a.coverage.shape
            fonts["glyph_first"][f], fonts["n_classes"][f] = first, a.n_classes
            first += a.n_classes
        self.n_pairs = first
        staged, _ = Staging().stage(0, lay)
        self.resident = upload(staged, self.device)
        self.pairs_off, self.fonts_off = lay.offsets[-2:]
        self._staging = Staging()
        self._copied = [None, None]             # per staging slot: the event behind the last H2D copy out of it
        self._slot = 0

    def render(self, items, canvases, H, W, u8=False, f32=True, extra=()):
        """items: ITEM_DTYPE array, canvases: CANVAS_DTYPE array (photo_off relative to `self.resident`), extra: further
        numpy sections for the same staging copy.  Returns (u8 [N, H, W, 3] or None, f32 [N, 3, H, W] or None, the device
        buffer, the offsets of `extra` in it).
        The H2D copy is asynchronous and the stream may be far behind the host (a generator runs ahead of the training step), so
        the pinned bytes of a call must not be rewritten before its copy has run: two slots alternate, and a slot is staged again
        only after the event recorded behind its last copy (the host then waits for the copy of the call before last, no more)."""
        n = len(canvases)
        lay = Sections([items if len(items) else 16, canvases if n else 16] + list(extra), pad_end=True)
        slot, self._slot = self._slot, self._slot ^ 1
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()
        staged, _ = self._staging.stage(slot, lay)
        dbuf = upload(staged, self.device)
        if self.device.type == "cuda":
            self._copied[slot] = torch.cuda.Event()
            self._copied[slot].record(torch.cuda.current_stream(self.device))
        out_u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device) if u8 else None
        out_f32 = torch.empty((n, 3, H, W), dtype=torch.float32, device=self.device) if f32 else None
        base = self.resident.data_ptr()
        call("mr_synth_render", base, base + self.fonts_off, len(self.atlases), base + self.pairs_off, self.n_pairs,
             dbuf.data_ptr() + lay.offsets[0], len(items), dbuf.data_ptr() + lay.offsets[1], n, H, W,
             RGB_MEAN[0], RGB_MEAN[1], RGB_MEAN[2], ptr(out_u8), ptr(out_f32))
        return out_u8, out_f32, dbuf, lay.offsets[2:]


class _Words(object):
    """Word source: a list (drawn uniformly) or a callable rng -> str.  A word that is empty, longer than `max_size` or has a
    character without a glyph in the font drawn with it is drawn again, at most TRIES times a word.  For a list the rejection is
    worked out once: drawing again until a (word, font) pair can be drawn is drawing uniformly from the pairs that can."""
    TRIES = 100

    def __init__(self, charset, atlases, words, max_size):
        self.charset, self.atlases, self.max_size = charset, atlases, min(int(max_size), MAX_GLYPHS)
        self.gh = np.array([a.gh for a in atlases], dtype=np.float64)
        self.words = words if callable(words) else list(words)
        if callable(words):
            return
        if not self.words:
            raise ValueError("synthetic text needs words")
        ids = np.zeros((len(self.words), MAX_GLYPHS), dtype=np.int32)
        count = np.zeros(len(self.words), dtype=np.int32)
        pairs, widths = [], []
        for k, word in enumerate(self.words):
            if not 0 < len(word) <= self.max_size:
                continue
            count[k] = len(word)
            ids[k, :len(word)] = [charset.index(ch) for ch in word]
            for f, atlas in enumerate(atlases):
                if atlas.has_glyph(ids[k, :len(word)]).all():
                    pairs.append((k, f))
                    widths.append(atlas.w[ids[k, :len(word)]].sum())
        if not pairs:
            raise ValueError("no drawable word: every word is empty, longer than %d characters or has a character without a "
                             "glyph in every font" % self.max_size)
        self.ids, self.count = ids, count
        self.pairs, self.widths = np.array(pairs, dtype=np.int32), np.array(widths, dtype=np.float64)

    def draw(self, rng, n):
        """n words: (texts, font [n], glyph ids [n, MAX_GLYPHS], counts [n], line widths [n], line heights [n])."""
        if not callable(self.words):
            pick = rng.integers(len(self.pairs), size=n)
            word, font = self.pairs[pick, 0], self.pairs[pick, 1]
            return [self.words[k] for k in word], font, self.ids[word], self.count[word], self.widths[pick], self.gh[font]
        texts, font = [], np.zeros(n, dtype=np.int32)
        ids, count, widths = np.zeros((n, MAX_GLYPHS), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
        for k in range(n):
            for _ in range(self.TRIES):
                word, f = self.words(rng), int(rng.integers(len(self.atlases)))
                g = [self.charset.index(ch) for ch in word]
                if 0 < len(word) <= self.max_size and self.atlases[f].has_glyph(g).all():
                    break
            else:
                raise ValueError("no drawable word in %d tries: every word is empty, longer than %d characters or has a "
                                 "character without a glyph" % (self.TRIES, self.max_size))
            texts.append(word)
            font[k], count[k], widths[k] = f, len(g), self.atlases[f].w[g].sum()
            ids[k, :len(g)] = g
        return texts, font, ids, count, widths, self.gh[font]


class SynthText(object):
    """An endless stream of labelled word crops with the keys, dtypes and shapes of `DevicePipeline.process`."""

    def __init__(self, charset, atlases, words, image_size=(32, 128), style=None, seed=0, max_size=32, device=None):
        self.charset = charset if charset is not None else EnglishCharset()
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.style = style if style is not None else SynthStyle()
        self.seed, self.max_size = int(seed), int(max_size)
        self.atlases = list(atlases)
        self._words = _Words(self.charset, self.atlases, words, min(self.max_size, MAX_GLYPHS))
        self._renderer = None
        self._device = device
        self.index = 0

    def plan(self, n, index):
        """Host side: (items, canvases, quads [n, 4, 2], texts) of batch number `index`; a function of (seed, index, n) alone."""
        rng = np.random.default_rng([self.seed, int(index)])
        H, W = self.image_size
        style = self.style
        texts, font, glyphs, counts, lw, gh = self._words.draw(rng, n)
        half_h = rng.uniform(style.height[0], style.height[1], n) * H / 2.0
        half_w = rng.uniform(style.width[0], style.width[1], n) * W / 2.0
        cx = W / 2.0 + rng.uniform(-1.0, 1.0, n) * (W / 2.0 - half_w)
        cy = H / 2.0 + rng.uniform(-1.0, 1.0, n) * (H / 2.0 - half_h)
        quads = word_quads(rng, style, cx, cy, half_w, half_h, H, W)
        canvases = np.zeros(n, dtype=CANVAS_DTYPE)
        canvases["first_item"], canvases["n_items"] = np.arange(n), 1
        bg0, bg1 = fill_canvases(canvases, rng, style, H, W)
        items = np.zeros(n, dtype=ITEM_DTYPE)
        fill_items(items, rng, style, np.arange(n), font, glyphs, counts, lw, gh, quads, H, W)
        shadow_colours(items, contrasting(rng, style, (bg0 + bg1) / 2.0), (bg0 + bg1) / 2.0)
        return items, canvases, quads, texts

    def batch(self, n, index=None, photos=False):
        """{'image' f32 [n, 3, H, W], 'label' i32 [n, max_size], 'length' i32 [n], 'text': list of str} on the device, plus
        'photos' u8 [n, H, W, 3] on request.  index: the batch number (default: the next one)."""
        if index is None:
            index, self.index = self.index, self.index + 1
        if self._renderer is None:
            self._renderer = SynthRenderer(self.atlases, self._device)
        items, canvases, quads, texts = self.plan(n, index)
        # the glyph ids ARE the charset's encoding of the text: `_Words` made them with charset.index, as `string_to_label` does
        width = min(self.max_size, MAX_GLYPHS)
        label = np.zeros((n, self.max_size), dtype=np.int32)
        label[:, :width] = items["glyph"][:, :width]
        length = np.minimum(items["n_glyphs"], self.max_size).astype(np.int32)
        H, W = self.image_size
        u8, f32, dbuf, (label_off, length_off) = self._renderer.render(items, canvases, H, W, u8=photos, f32=True,
                                                                       extra=[label.reshape(-1), length])
        out = {'image': f32,
               'label': dbuf[label_off:label_off + label.nbytes].view(torch.int32).view(n, self.max_size),
               'length': dbuf[length_off:length_off + length.nbytes].view(torch.int32),
               'text': texts, '_keepalive': dbuf}
        if photos:
            out['photos'] = u8
        return out

    batch_size = 256                    # of the batches `__iter__` yields

    def __iter__(self):
        """Endless: batch after batch of `batch_size` crops."""
        while True:
            yield self.batch(self.batch_size)


class SynthScenes(object):
    """Labelled scenes: several words on a larger canvas, their quadrilaterals and texts.  Words are placed without overlap by
    bounded rejection (at most 20 tries a word, then the scene has fewer words).  backgrounds: optional resident uint8 HWC
    CUDA tensors of at least the canvas size, one drawn per scene."""
    PLACE_TRIES = 20

    def __init__(self, charset, atlases, words, canvas=(640, 640), words_per_scene=(1, 12), style=None, seed=0, max_size=32,
                 backgrounds=None, device=None):
        self.charset = charset if charset is not None else EnglishCharset()
        self.canvas = (int(canvas[0]), int(canvas[1]))
        self.words_per_scene = (int(words_per_scene[0]), int(words_per_scene[1]))
        if not 0 <= self.words_per_scene[0] <= self.words_per_scene[1] <= MAX_ITEMS:
            raise ValueError("words_per_scene must be a range inside [0, %d], got %s" % (MAX_ITEMS, words_per_scene))
        self.style = style if style is not None else SynthStyle()
        self.seed = int(seed)
        self.atlases = list(atlases)
        self._words = _Words(self.charset, self.atlases, words, max_size)
        self.backgrounds = list(backgrounds) if backgrounds else []
        for b in self.backgrounds:
            if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.uint8 and b.dim() == 3 and b.shape[2] == 3
                    and b.shape[0] >= self.canvas[0] and b.shape[1] >= self.canvas[1] and b.stride(2) == 1
                    and b.stride(1) == 3):
                raise TypeError("backgrounds are resident uint8 HWC CUDA tensors of at least the canvas size")
        self._renderer = None
        self._device = device
        self.index = 0

    def plan(self, n, index):
        """Host side: (items, canvases, quads [I, 4, 2] in item order, texts per scene, background index per scene or None).
        Every word's PLACE_TRIES candidate places are drawn at once; only the choice among them runs word by word."""
        rng = np.random.default_rng([self.seed, int(index)])
        H, W = self.canvas
        style, T = self.style, self.PLACE_TRIES
        canvases = np.zeros(n, dtype=CANVAS_DTYPE)
        bg0, bg1 = fill_canvases(canvases, rng, style, H, W)
        back = rng.integers(len(self.backgrounds), size=n) if self.backgrounds else None
        want = rng.integers(self.words_per_scene[0], self.words_per_scene[1] + 1, size=n)
        total = int(want.sum())
        texts, font, glyphs, counts, lw, gh = self._words.draw(rng, total)
        half_h = rng.uniform(style.scene_height[0], style.scene_height[1], (total, T)) * H / 2.0
        half_w = half_h * (lw / gh)[:, None]
        cand = word_quads(rng, style, rng.uniform(0.0, W, total * T), rng.uniform(0.0, H, total * T), half_w.reshape(-1),
                          half_h.reshape(-1), H, W).reshape(total, T, 4, 2)
        lo, hi = cand.min(axis=2).tolist(), cand.max(axis=2).tolist()
        keep, place = [], []
        word = 0
        for s in range(n):
            boxes = []
            canvases["first_item"][s] = len(keep)
            for _ in range(int(want[s])):
                for t in range(T):
                    (x0, y0), (x1, y1) = lo[word][t], hi[word][t]
                    if all(x0 >= b[2] or x1 <= b[0] or y0 >= b[3] or y1 <= b[1] for b in boxes):
                        boxes.append((x0, y0, x1, y1))
                        keep.append(word)
                        place.append(t)
                        break
                word += 1
            canvases["n_items"][s] = len(keep) - canvases["first_item"][s]
        keep, place = np.array(keep, dtype=np.int64), np.array(place, dtype=np.int64)
        I = len(keep)
        scene = np.repeat(np.arange(n), canvases["n_items"]).astype(np.int32)
        quads = cand[keep, place].reshape(I, 4, 2)
        items = np.zeros(I, dtype=ITEM_DTYPE)
        fill_items(items, rng, style, scene, font[keep], glyphs[keep], counts[keep], lw[keep], gh[keep], quads, H, W)
        ground = (bg0[scene] + bg1[scene]) / 2.0 if back is None else np.full((I, 3), 127.5)
        shadow_colours(items, contrasting(rng, style, ground), ground)
        kept = [texts[k] for k in keep]
        ends = np.cumsum(canvases["n_items"])
        return items, canvases, quads, [kept[e - c:e] for e, c in zip(ends.tolist(), canvases["n_items"].tolist())], back

    def batch(self, n, index=None):
        """{'photos': u8 [n, H, W, 3] on the device (B, G, R), 'polygons': list of float64 [K, 4, 2], 'ignore_tags': list of bool
        [K], 'texts': list of lists of str}."""
        if index is None:
            index, self.index = self.index, self.index + 1
        if self._renderer is None:
            self._renderer = SynthRenderer(self.atlases, self._device)
        items, canvases, quads, texts, back = self.plan(n, index)
        if back is not None:
            base = self._renderer.resident.data_ptr()
            for s in range(n):
                b = self.backgrounds[int(back[s])]
                canvases["photo"][s], canvases["photo_pitch"][s] = 1, b.stride(0)
                canvases["photo_off"][s] = b.data_ptr() - base
        H, W = self.canvas
        u8, _, dbuf, _ = self._renderer.render(items, canvases, H, W, u8=True, f32=False)
        polygons, tags = [], []
        for s in range(n):
            first, cnt = int(canvases["first_item"][s]), int(canvases["n_items"][s])
            polygons.append(np.array([order_quad(q) for q in quads[first:first + cnt]], dtype=np.float64).reshape(cnt, 4, 2))
            tags.append(np.zeros(cnt, dtype=bool))
        return {'photos': u8, 'polygons': polygons, 'ignore_tags': tags, 'texts': texts, '_keepalive': dbuf}
