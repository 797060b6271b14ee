"""Window geometry of MultiDiffusion sampling (Bar-Tal et al., ICML 2023; diffusers StableDiffusionPanoramaPipeline): a canvas
larger than the UNet's window is covered by overlapping S x S windows, which are all the model ever sees.  Host only, pure Python:
the kernels (csrc/pano.hip: afldm_pano_step, afldm_window_fuse, afldm_window_crop) take the origin lists this module makes, the
engine (engine.PanoramaEngine) keys its cache on the Geometry.

Per axis, `window_origins(extent, S, stride, circular)`:
    not circular:  0, stride, 2 stride, ... while o + S < extent, then a last window flush at extent - S (the last gap may be
                   shorter than `stride`); extent == S gives (0,)
    circular:      k stride for k < ceil(extent / stride); the window covers (o + u) mod extent
A 2-D grid is the product of the two lists, window k = iy * nx + ix.  At most MAX_ORIGINS windows per axis.

`place(Hc, Wc, S, top, left, margin, wrap_x)` is where a window-sized block given to MyLDMPipeline.outpaint lies on the canvas: the
rows and columns of the paste and of the kept rectangle, and the canvas mask."""
from dataclasses import dataclass

MAX_ORIGINS = 16


def window_origins(extent, S, stride, circular=False):
    extent, S, stride = int(extent), int(S), int(stride)
    if S < 1 or extent < S:
        raise ValueError(f"window_origins: a window of {S} on an axis of extent {extent}")
    if not 1 <= stride <= S:
        raise ValueError(f"window_origins: stride {stride} must be in [1, {S}]: a larger one leaves gaps")
    if circular:
        origins = tuple(k * stride for k in range(-(-extent // stride)))
    else:
        origins, o = [], 0
        while o + S < extent:
            origins.append(o)
            o += stride
        origins = tuple(origins) + (extent - S,)
    if len(origins) > MAX_ORIGINS:
        raise ValueError(f"window_origins: {len(origins)} windows on an axis (extent {extent}, stride {stride}); at most {MAX_ORIGINS}")
    return origins


@dataclass(frozen=True)
class Geometry:
    """The windows of one canvas: extents, window size, the per-axis origin lists and which axes wrap.  Hashable: it is part of
    the engine cache key, since the captured graphs hold the origins."""
    Hc: int
    Wc: int
    S: int
    oy: tuple
    ox: tuple
    wrap_y: bool = False
    wrap_x: bool = False

    @classmethod
    def grid(cls, Hc, Wc, S, stride_y, stride_x, circular_x=False, circular_y=False):
        return cls(int(Hc), int(Wc), int(S), window_origins(Hc, S, stride_y, circular_y), window_origins(Wc, S, stride_x, circular_x),
                   bool(circular_y), bool(circular_x))

    @property
    def ny(self):
        return len(self.oy)

    @property
    def nx(self):
        return len(self.ox)

    @property
    def nwin(self):
        return len(self.oy) * len(self.ox)

    def scaled(self, r):
        """The same windows in units r times finer (latents -> pixels of a VAE with scale factor r)."""
        r = int(r)
        return Geometry(self.Hc * r, self.Wc * r, self.S * r, tuple(o * r for o in self.oy), tuple(o * r for o in self.ox),
                        self.wrap_y, self.wrap_x)

    def corners(self):
        """(oy, ox) of window k = iy * nx + ix, in k order."""
        return [(y, x) for y in self.oy for x in self.ox]


@dataclass(frozen=True)
class Placement:
    """Where an S x S block lies on a canvas (place): the canvas rows and columns of its S rows and columns, in block order, and
    those of the kept rectangle - the block shrunk by `margin` on each side."""
    top: int
    left: int
    rows: tuple
    cols: tuple
    keep_rows: tuple
    keep_cols: tuple

    def mask(self, Hc, Wc):
        """The canvas mask as Hc lists of Wc floats: 1.0 on the kept rectangle, 0.0 elsewhere."""
        rows, cols = set(self.keep_rows), set(self.keep_cols)
        return [[1.0 if y in rows and x in cols else 0.0 for x in range(int(Wc))] for y in range(int(Hc))]


def place(Hc, Wc, S, top=None, left=None, margin=0, wrap_x=False):
    """The Placement of an S x S block with its corner at (top, left) on an Hc x Wc canvas, all in the canvas's units (the paste and
    the mask of MyLDMPipeline.outpaint).  None centres the block on that axis.  On a wrapping x axis `left` may be anywhere in
    [0, Wc) and the columns are taken modulo Wc; otherwise the block has to lie inside the canvas.  `margin`: the kept rectangle
    is the block without its outer `margin` rows and columns.  Raises ValueError for a position off the grid (not an integer)
    or outside the canvas, and for a margin that leaves nothing."""
    Hc, Wc, S = int(Hc), int(Wc), int(S)
    if S < 1 or S > Hc or S > Wc:
        raise ValueError(f"place: a block of {S} on a {Hc} x {Wc} canvas")
    top = (Hc - S) // 2 if top is None else top
    left = (Wc - S) // 2 if left is None else left
    for name, v in (("top", top), ("left", left), ("margin", margin)):
        if int(v) != v:
            raise ValueError(f"place: {name} = {v} is off the grid")
    top, left, margin = int(top), int(left), int(margin)
    if not 0 <= top <= Hc - S:
        raise ValueError(f"place: rows {top} .. {top + S - 1} leave the canvas of {Hc} rows")
    if not (0 <= left < Wc if wrap_x else 0 <= left <= Wc - S):
        raise ValueError(f"place: columns {left} .. {left + S - 1} leave the {'wrapping ' if wrap_x else ''}canvas of {Wc} columns")
    if margin < 0 or 2 * margin >= S:
        raise ValueError(f"place: a margin of {margin} leaves nothing of a block of {S}")
    rows = tuple(range(top, top + S))
    cols = tuple((left + v) % Wc for v in range(S))
    return Placement(top, left, rows, cols, rows[margin:S - margin], cols[margin:S - margin])


def feather(n):
    """The triangular window t[i] = min(i + 1, n - i), strictly positive, as a list of n floats: the separable blending weight of
    the per-window decodes (MyLDMPipeline.panorama)."""
    return [float(min(i + 1, n - i)) for i in range(int(n))]
