"""test.ipynb through the package aliases of INTEGRATION.md §2(a), `IQA_pytorch` included, and the batched `metrics.Evaluator`, in a child
process (as tests/test_gpu_model.py::test_notebook_flow_through_package_alias does for train.ipynb).

The numbers are held against the float64 restatement (tests/quality_ref.py) evaluated on the tensors the model itself produced — the
notebook's on `get_current_visuals()`, the evaluator's on what its `update` was handed — so the convolutions' run-to-run differences do
not enter: SSIM within 1e-6 for the notebook's float32 score, 1e-10 for the evaluator's float64 one (the kernel's bound,
tests/test_gpu_image_quality.py), PSNR to 1e-9 dB and the validation loss to 1e-12 relative (both follow from means good to 1e-12).
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import sys, os
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import deepinpainting_amd.models as _m, deepinpainting_amd.util as _u
sys.modules["models"], sys.modules["util"] = _m, _u
for _n in ("models", "IPSR", "IPSR_model", "IPSRFunction", "InnerCos", "InnerCos2", "networks", "base_model", "vgg16", "Early"):
    __import__("deepinpainting_amd.models." + _n); sys.modules["models." + _n] = sys.modules["deepinpainting_amd.models." + _n]
for _n in ("util", "NonparametricShift", "MaxCoord", "data_load", "ref_data_load"):
    __import__("deepinpainting_amd.util." + _n); sys.modules["util." + _n] = sys.modules["deepinpainting_amd.util." + _n]
import deepinpainting_amd.metrics
sys.modules.setdefault("IQA_pytorch", deepinpainting_amd.metrics)

# ---- test.ipynb cell 0 (the fields the models read; paths replaced)
class Option():
    def __init__(self):
        self.batchSize = 1; self.fineSize = 256; self.input_nc = 3; self.input_nc_g = 6; self.output_nc = 3
        self.ngf = 64; self.ndf = 64; self.which_model_netD = 'basic'; self.which_model_netF = 'feature'
        self.which_model_netG = 'unet_ipsr'; self.which_model_netP = 'unet_256'; self.triple_weight = 1
        self.name = 'IPSR_inpainting'; self.n_layers_D = '3'; self.gpu_ids = [0]; self.model = 'ipsr_net'
        self.checkpoints_dir = %(ckpt)r; self.norm = 'instance'; self.fixed_mask = 1; self.use_dropout = False
        self.init_type = 'normal'; self.mask_type = 'random'; self.lambda_A = 100; self.threshold = 5 / 16.0
        self.stride = 1; self.shift_sz = 1; self.mask_thred = 1; self.bottleneck = 512; self.gp_lambda = 10.0
        self.ncritic = 5; self.constrain = 'MSE'; self.strength = 1; self.init_gain = 0.02; self.cosis = 1
        self.gan_type = 'lsgan'; self.gan_weight = 0.2; self.overlap = 4; self.skip = 0; self.continue_train = False
        self.epoch_count = 1; self.phase = 'train'; self.which_epoch = 1; self.niter = 20; self.niter_decay = 100
        self.beta1 = 0.5; self.lr = 0.0002; self.lr_policy = 'lambda'; self.lr_decay_iters = 50; self.isTrain = False

# ---- cell 1 (the imports the notebook makes from the aliased packages)
from util.data_load import Data_load
from models.models import create_model
import torch
from IQA_pytorch import SSIM
import numpy as np
import quality_ref as R

# a checkpoint for cell 2's load: the trainer, built once, saved as epoch 1
topt = Option(); topt.isTrain = True; topt.which_epoch = ''; topt.use_dropout = True; topt.quiet = True
create_model(topt).save(1)
opt = Option()
model = create_model(opt)
model.load(1)

# ---- cell 3, loop body (one synthetic batch instead of the DataLoader; the picture is not written)
g = torch.Generator().manual_seed(3)
image = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
mask = torch.zeros(1, 1, 256, 256); mask[:, :, 40:200, 90:170] = 1
image=image.cuda()
mask=mask.cuda()
mask=mask[0][0]
mask=torch.unsqueeze(mask,0)
mask=torch.unsqueeze(mask,1)
mask=mask.bool()

model.set_input(image,mask,image) # it not only sets the input data with mask, but also sets the latent mask.
model.set_ref_latent()
model.set_gt_latent()
model.test()

real_A,ref_B,fake_B,fake_P,real_B=model.get_current_visuals()
pic = (torch.cat([real_A,ref_B,fake_P,fake_B], dim=0) + 1) / 2.0

psnr=0
mse=0
if type(real_B)==torch.Tensor:
    mse=torch.mean((real_B-fake_B)**2)
else:
    mse=np.mean((real_B-fake_B)**2)

if mse==0:
    psnr=100
else:
    psnr=10*torch.log10((2**2)/mse)
errors=model.get_error()

mod=SSIM(channels=3)
score=mod(real_B,fake_B,as_loss=False)
print('%%d. PSNR : %%f, SSIM : %%f' %%(1,psnr,score))
# ---- end of the notebook's code
assert type(mod) is deepinpainting_amd.metrics.SSIM and score.shape == (1,) and score.dtype == torch.float32
assert np.isfinite(float(psnr)) and pic.shape == (4, 3, 256, 256)
want = R.ssim(real_B, fake_B)
err = abs(float(score) - float(want))
print("notebook SSIM %%.8f restatement %%.8f |diff| %%.2e" %% (float(score), float(want), err))
assert err <= 1e-6, err

# ---- the same loop in batches: three images, three holes, one host read
from deepinpainting_amd.metrics import Evaluator
images = torch.rand(3, 3, 256, 256, generator=g).cuda() * 2 - 1
masks = torch.zeros(3, 1, 256, 256, dtype=torch.bool, device="cuda")
masks[0, :, 40:200, 90:170] = True; masks[1, :, 100:140, 30:220] = True; masks[2, :, 16:80, 16:80] = True
ev = Evaluator(model)
seen, returned = [], []
inner = ev.update
def spy(real_B, fake_B, fake_P=None):
    seen.append((real_B.detach().clone(), fake_B.detach().clone(), fake_P.detach().clone()))
    returned.append(inner(real_B, fake_B, fake_P))
ev.update = spy
with torch.enable_grad():
    ev.step(images, masks, images)
assert returned == [None] and len(seen) == 1 and seen[0][0].shape == (3, 3, 256, 256)
assert not model.fake_B.requires_grad                                   # step ran under no_grad
held = [t for t in ev._quality + ev._l1_P]
assert held and all(torch.is_tensor(t) and t.is_cuda for t in held)
res = ev.result()
rB, fB, fP = seen[0]
q, qP = R.quality(rB, fB), R.quality(fP, rB, with_ssim=False)
e_ssim = float(np.abs(res["ssim"] - q[:, 0].numpy()).max())
e_psnr = float(np.abs(res["psnr"] - R.psnr_of_mse(q[:, 1]).numpy()).max())
vl = ((q[:, 2] + qP[:, 2]) * 100.0).numpy()
e_vl = float(np.abs(res["valid_loss"] / vl - 1).max())
print("evaluator: |SSIM - ref| %%.2e, |PSNR - ref| %%.2e dB, valid loss rel %%.2e; SSIM %%s PSNR %%s" %% (e_ssim, e_psnr, e_vl, res["ssim"], res["psnr"]))
assert res["images"] == 3 and res["ssim"].shape == res["psnr"].shape == res["valid_loss"].shape == (3,)
assert e_ssim <= 1e-10 and e_psnr <= 1e-9 and e_vl <= 1e-12
assert abs(res["ssim_average"] - res["ssim"].mean()) <= 1e-15 and abs(res["psnr_average"] - res["psnr"].mean()) <= 1e-12
assert abs(res["valid_loss_average"] - res["valid_loss"].mean()) <= 1e-12
assert len(set(np.round(res["ssim"], 6))) == 3                           # three images, three holes: three different scores
# ---- cell 3 as one call: a DataLoader-like iterator of CPU batches, masks as ToTensor gives them (float, three channels); stops at max_images
from deepinpainting_amd.metrics import evaluate
fmask = masks.float().cpu().expand(3, 3, 256, 256)
r2 = evaluate(model, iter([(images.cpu(), fmask, images.cpu()), (images.cpu(), fmask, images.cpu())]), max_images=5)
assert r2["images"] == 5 and np.isfinite(r2["psnr"]).all() and np.isfinite(r2["ssim"]).all() and np.isfinite(r2["valid_loss"]).all()
print("EVAL_FLOW_OK")
"""


@pytest.mark.gpu
def test_test_notebook_and_batched_evaluator_through_the_aliases(tmp_path):
    script = SCRIPT % {"root": ROOT, "ckpt": str(tmp_path)}
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert "EVAL_FLOW_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
