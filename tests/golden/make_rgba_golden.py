"""Records tests/golden/rgba_golden.npz: what the reference's own RGBA preprocessing returns for one small soft-edged image.

    python tests/golden/make_rgba_golden.py /path/to/the/reference/checkout

Imports `TrellisImageTo3DPipeline.preprocess_image` (trellis/pipelines/trellis_image_to_3d.py) and `remove_background`
(scripts/encode_in_the_wild_img_cond_dinov2_feature.py) from that checkout, with empty stand-ins for the modules they import but do not
use on an image that carries alpha (rembg, the TRELLIS package around the pipeline, imageio ...), runs them with Pillow and numpy, and
stores the input, the boxes and a SHA-256 of each output array: recorded results only."""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import rgba_ref as R  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a harmless callable class."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if f"{self.__name__}.{name}" in sys.modules:
            return sys.modules[f"{self.__name__}.{name}"]
        return type(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: None})


def stub(*names):
    for n in names:
        if n not in sys.modules:
            sys.modules[n] = _Anything(n)


def have(name):
    try:
        return importlib.util.find_spec(name) is not None
    except (ImportError, ValueError):
        return False


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    stub("rembg", "trellis", "trellis.pipelines", "trellis.pipelines.base", "trellis.pipelines.samplers", "trellis.modules", "trellis.modules.sparse",
         "trellis.representations")
    for opt in ("easydict", "tqdm", "torchvision", "torchvision.transforms", "imageio", "pandas"):
        if not have(opt.split(".")[0]):
            stub(opt)
    pipe = load("trellis.pipelines.trellis_image_to_3d", os.path.join(ref, "trellis", "pipelines", "trellis_image_to_3d.py"))
    wild = load("gvf_ref_wild_script", os.path.join(ref, "scripts", "encode_in_the_wild_img_cond_dinov2_feature.py"))

    img = R.soft_disc(48, 64, 2024)
    pil = Image.fromarray(img)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    a = np.asarray(pipe.TrellisImageTo3DPipeline.preprocess_image(types.SimpleNamespace(), pil))
    b_image, b_box, b_mask = wild.remove_background(pil)
    b_image, b_mask = np.asarray(b_image), np.asarray(b_mask)
    np.savez_compressed(os.path.join(HERE, "rgba_golden.npz"), input=img, a_shape=np.asarray(a.shape), a_sha256=sha(a),
                        b_box=np.asarray([float(v) for v in b_box]), b_image_sha256=sha(b_image), b_mask_sha256=sha(b_mask))
    print("A", a.shape, sha(a)[:16], "B", b_image.shape, b_mask.shape, [float(v) for v in b_box])


if __name__ == "__main__":
    main(sys.argv[1])
