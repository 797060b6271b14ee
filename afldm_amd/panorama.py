"""Window geometry of MultiDiffusion sampling (Bar-Tal et al., ICML 2023; diffusers StableDiffusionPanoramaPipeline): a canvas
larger than the UNet's window is covered by overlapping S x S windows, which are all the model ever sees.  Host only, pure Python:
the kernels (csrc/pano.hip: afldm_pano_step, afldm_window_fuse, afldm_window_crop) take the origin lists this module makes, the
engine (engine.PanoramaEngine) keys its cache on the Geometry.

Per axis, `window_origins(extent, S, stride, circular)`:
    not circular:  0, stride, 2 stride, ... while o + S < extent, then a last window flush at extent - S (the last gap may be
                   shorter than `stride`); extent == S gives (0,)
    circular:      k stride for k < ceil(extent / stride); the window covers (o + u) mod extent
A 2-D grid is the product of the two lists, window k = iy * nx + ix.  At most MAX_ORIGINS windows per axis."""
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


def feather(n):
    """The triangular window t[i] = min(i + 1, n - i), strictly positive, as a list of n floats: the separable blending weight of
    the per-window decodes (MyLDMPipeline.panorama)."""
    return [float(min(i + 1, n - i)) for i in range(int(n))]
