"""Generates tests/golden/lpips_golden.npz by running the REFERENCE's LPIPS forward (utils/lpips/lpips.py:LPIPS.forward over
utils/lpips/networks.py:BaseNet.forward and LinLayers, utils/lpips/utils.py:normalize_activation), on the CPU in float64, with the
weights of tests/lpips_ref.py:seeded_weights.  Runs only in the build container, like make_ssim_golden.py.
Usage:  python tests/golden/make_lpips_golden.py

Nothing is downloaded and no pretrained network is built: the reference's LPIPS, VGG16 and get_state_dict constructors are never
called.  A throw-away `torchvision` module stands in for the import at the top of networks.py; the trunk is a subclass of the
reference's BaseNet whose `layers` is a locally built nn.Sequential in vgg16.features order with target_layers [4, 9, 16, 23, 30];
LPIPS.forward is called unbound on a plain object that carries .net and .lin.  As a guard, torch.hub.load_state_dict_from_url raises.

Per case k: x_k, y_k (fp32 inputs), loss_k (the fp64 loss), grad_k (its fp64 gradient in x).  `seed`: the weights' seed."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_ref  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "lpips_golden.npz")
SEED = 7
SHAPES = [(2, 3, 37, 50), (1, 3, 16, 16)]
VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


def _no_download(*a, **k):
    raise RuntimeError("make_lpips_golden: nothing may be downloaded")


def load_reference():
    torch.hub.load_state_dict_from_url = _no_download
    sys.modules.setdefault("torchvision", types.SimpleNamespace(models=types.SimpleNamespace()))
    pkg = types.ModuleType("ref_lpips")
    pkg.__path__ = [f"{REF}/utils/lpips"]
    sys.modules["ref_lpips"] = pkg
    mods = {}
    for name in ("utils", "networks", "lpips"):
        spec = importlib.util.spec_from_file_location(f"ref_lpips.{name}", f"{REF}/utils/lpips/{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"ref_lpips.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def features():
    layers, cin = [], 3
    for v in VGG_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def main():
    ref = load_reference()

    class Trunk(ref["networks"].BaseNet):
        def __init__(self):
            super().__init__()
            self.layers = features()
            self.target_layers = [4, 9, 16, 23, 30]

    sd = lpips_ref.seeded_weights(SEED)
    net, lin = Trunk(), ref["networks"].LinLayers([64, 128, 256, 512, 512])
    holder = nn.Module()
    holder.net, holder.lin = net, lin
    holder.load_state_dict(sd, strict=True)
    holder.double()
    data = {"seed": np.array(SEED)}
    for k, shape in enumerate(SHAPES):
        x, y = lpips_ref.seeded_images(100 + k, shape)
        xr = x.double().requires_grad_(True)
        loss = ref["lpips"].LPIPS.forward(holder, xr, y.double())
        loss.backward()
        data[f"x_{k}"], data[f"y_{k}"] = x.numpy(), y.numpy()
        data[f"loss_{k}"], data[f"grad_{k}"] = loss.detach().numpy(), xr.grad.numpy()
        print(shape, float(loss), float(xr.grad.abs().max()))
    data["n_cases"] = np.array(len(SHAPES))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
