#!/usr/bin/env python3
"""Bit identity of the fused execution (models/fused.py) between two source trees: SHA-256 of the four nets' outputs and of every
parameter gradient, for the model of tests/test_gpu_model.py::test_fused_sequential_matches_plain_modules.

    python tools/ab_fused_exec.py --tree <checkout of the parent commit, libipsr_hip.so built or copied in> > parent.txt
    python tools/ab_fused_exec.py --tree . > new.txt
    diff parent.txt new.txt            # no line may differ (profiles/fused_exec_ab.txt)

One process per tree (the package is imported from --tree).  Three passes: fp32 with FusedSequential.skip_source on and off, and
the trainer under bf16 autocast as `bench.py --dtype bf16` sets it (Option(amp_bf16=True)).  Each is a forward and the backward
of the sum of squares of fake_B, fake_P, netD(fake_B), netF(relu3_3).
"""
import argparse
import contextlib
import hashlib
import io
import os
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path[:0] = [tree, os.path.join(tree, "tests")]
os.environ.setdefault("IPSR_ALLOW_RANDOM_VGG", "1")

import torch  # noqa: E402
import golden_cases  # noqa: E402
import deepinpainting_amd  # noqa: E402
from deepinpainting_amd.models.fused import FusedSequential  # noqa: E402
from deepinpainting_amd.models.models import create_model  # noqa: E402
from deepinpainting_amd.options import Option  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(deepinpainting_amd.__file__))) == tree
torch.backends.cudnn.deterministic = True


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def one_pass(tag, amp_bf16, skip_source):
    with tempfile.TemporaryDirectory() as ck, contextlib.redirect_stdout(io.StringIO()):
        m = create_model(Option(gpu_ids=[0], batchSize=2, use_dropout=False, quiet=True, triple_weight=0.0, amp_bf16=amp_bf16, checkpoints_dir=ck))
    for i, net in enumerate((m.netG, m.netP, m.netD, m.netF, m.vgg)):
        golden_cases.reinit_deterministic(net, 900 + i)
    img, mask, ref = golden_cases.trainer_inputs(B=2)
    FusedSequential.skip_source = skip_source
    try:
        m.set_input(img.cuda(), mask.cuda(), ref.cuda())
        m.set_ref_latent()
        m.set_gt_latent()
        m.forward()
        with m._amp():
            pd = m.netD(m.fake_B)
            pf = m.netF(m._gt_latent.relu3_3)
        out = dict(fake_B=m.fake_B, fake_P=m.fake_P, pd=pd, pf=pf)
        sum((v.float() ** 2).mean() for v in out.values()).backward()
    finally:
        FusedSequential.skip_source = True
    torch.cuda.synchronize()
    for k, v in out.items():
        print(tag, k, str(v.dtype).replace("torch.", ""), sha(v))
    n = 0
    for name in ("netG", "netP", "netD", "netF"):
        for k, p in getattr(m, name).named_parameters():
            if p.grad is not None:
                print(tag, "grad:%s.%s" % (name, k), sha(p.grad))
                n += 1
    assert n > 100, n


one_pass("fp32/skip_source=1", False, True)
one_pass("fp32/skip_source=0", False, False)
one_pass("bf16/skip_source=1", True, True)
