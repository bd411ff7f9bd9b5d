#!/usr/bin/env python3
"""Generate tests/golden/g10_monodepth2.npz from the REFERENCE's own ResnetEncoder + DepthDecoder (the monodepth2 depth network of
MODEL.depth_network: monodepth2) and its convert_disp_to_depth.

Run in the build container only (needs the reference checkout, see make_golden.py):
    python tests/golden/make_golden_monodepth2.py

The loading of the reference by path, the torchvision stand-in and the test image are make_golden.py's.  The fixture holds inputs and
recorded results only: one 64x96 image, the four sigmoid disparities, one fixed random weight map per scale, the gradient norm of every
parameter under sum_s (disp_s * wgt_s).sum(), the first 16 gradient values of a few tensors and the depth of scale 0."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_reference, odn, save, smooth_image  # noqa: E402

SAMPLED = ("encoder.encoder.conv1.weight", "encoder.encoder.bn1.weight", "encoder.encoder.layer4.1.conv2.weight",
           "decoder.decoder.0.conv.conv.weight", "decoder.decoder.9.conv.conv.bias", "decoder.decoder.10.conv.weight",
           "decoder.decoder.11.conv.weight", "decoder.decoder.12.conv.weight", "decoder.decoder.13.conv.weight")


def main():
    _, _, tu, net = load_reference()
    torch.set_num_threads(8)
    H, W = 64, 96
    sd = odn.random_state_dict(0)
    enc = net.ResnetEncoder(18, False)
    dec = net.DepthDecoder(enc.num_ch_enc, range(4))
    parts = {"encoder.": enc, "decoder.": dec}
    for prefix, m in parts.items():
        res = m.load_state_dict(OrderedDict((k[len(prefix):], v) for k, v in sd.items() if k.startswith(prefix)))
        assert not res.missing_keys and not res.unexpected_keys, res
        m.eval()
    g = torch.Generator().manual_seed(31)
    img = smooth_image(H, W, g)
    out = dec(enc(img), 0)
    disps = [out[("disp", 0, s)] for s in range(4)]
    assert list(out.keys()) == [("disp", 0, s) for s in (3, 2, 1, 0)]
    wgts = [torch.rand(d.shape, generator=g) for d in disps]
    sum((d * w).sum() for d, w in zip(disps, wgts)).backward()
    params = OrderedDict((prefix + n, p) for prefix, m in parts.items() for n, p in m.named_parameters())
    gnorm = OrderedDict((n, (p.grad.norm() if p.grad is not None else torch.tensor(-1.0))) for n, p in params.items())
    depth0 = tu.convert_disp_to_depth(disps[0].detach(), 0.1, 80.0)
    save("g10_monodepth2", img=img, depth0=depth0, grad_names=np.array(list(gnorm.keys())), grad_norms=torch.stack(list(gnorm.values())),
         **{"disp%d" % s: d for s, d in enumerate(disps)}, **{"wgt%d" % s: w for s, w in enumerate(wgts)},
         **{"gs_" + k.replace(".", "_"): params[k].grad.flatten()[:16].clone() for k in SAMPLED})
    print("disparity ranges", [(round(float(d.detach().min()), 3), round(float(d.detach().max()), 3)) for d in disps],
          "parameters with a gradient:", sum(1 for v in gnorm.values() if v >= 0))


if __name__ == "__main__":
    main()
