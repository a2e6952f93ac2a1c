"""A word that follows a curve: `Ribbon(top, bottom)`, k rulings ordered along the reading direction, each a top point and a
bottom point in photo coordinates.  The word is the strip between the two polylines -- what DB's polygon output describes, what
CTW1500 and Total-Text annotate, what `mr_db_ribbons` (csrc/db_post.hip) reads off the detector's map and what `StripCropper`
(data/strip_crop.py) rectifies for the recogniser.  A box is the ribbon of two rulings (`from_box`)."""
import numpy as np

MAX_KNOTS = 18          # MR_RIBBON_MAX_KNOTS of include/megreader_hip.h: what one mr_strip_desc holds


class Ribbon(object):
    def __init__(self, top, bottom):
        self.top = np.array(top, dtype=np.float64)
        self.bottom = np.array(bottom, dtype=np.float64)
        if self.top.ndim != 2 or self.top.shape[1] != 2 or self.top.shape != self.bottom.shape:
            raise ValueError("Ribbon takes k top points and k bottom points [k, 2], got shapes %s and %s"
                             % (self.top.shape, self.bottom.shape))
        if not 2 <= len(self.top) <= MAX_KNOTS:
            raise ValueError("a ribbon has 2 to %d rulings, got %d" % (MAX_KNOTS, len(self.top)))

    @property
    def knots(self):
        return len(self.top)

    def polygon(self):
        """The outline [2 k, 2]: the top points forward, then the bottom points backward."""
        return np.concatenate([self.top, self.bottom[::-1]])

    def centres(self):
        return (self.top + self.bottom) / 2.0

    @classmethod
    def from_polygon(cls, points):
        """An even number of outline points, the first half the top, the second half the bottom reversed: the annotation order of
        CTW1500 and Total-Text, and what `polygon` returns."""
        p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        if len(p) % 2:
            raise ValueError("a ribbon's outline has an even number of points (top forward, bottom backward), got %d" % len(p))
        k = len(p) // 2
        return cls(p[:k], p[k:][::-1])

    @classmethod
    def from_box(cls, quad):
        """The two rulings whose strip crop is the quad crop of `quad` (`plan_crop` with 'min_area_rect'): its `rect_corners`
        TL, TR, BR, BL give top = (TL, TR) and bottom = (BL, BR); a vertical word (`plan_crop`'s `rotated` rule on the frame's
        integer sides) reads downwards with the crop's bottom on the photo's left, from the column cw - 1 of the frame that the
        quad crop's rotation starts at.  Raises DegenerateQuad for a zero side."""
        from ..data.quad_crop import DegenerateQuad, rect_corners         # (data.quad_crop imports this package)
        p = rect_corners(quad)
        w, h = float(np.linalg.norm(p[1] - p[0])), float(np.linalg.norm(p[2] - p[1]))
        if not (w > 0.0 and h > 0.0 and np.isfinite(w) and np.isfinite(h)):
            raise DegenerateQuad("ribbon: the quadrilateral %s has a zero side" % (np.asarray(quad).tolist(),))
        cw, ch = max(int(w), 1), max(int(h), 1)
        if ch > 1.5 * cw:
            t0 = p[0] + (p[1] - p[0]) / w * (cw - 1.0)
            t1 = t0 + (p[3] - p[0])
            return cls([t0, t1], [t0 - (p[1] - p[0]), t1 - (p[1] - p[0])])
        return cls([p[0], p[1]], [p[3], p[2]])

    def __eq__(self, other):
        return isinstance(other, Ribbon) and np.array_equal(self.top, other.top) and np.array_equal(self.bottom, other.bottom)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return "Ribbon(top=%s, bottom=%s)" % (self.top.tolist(), self.bottom.tolist())
