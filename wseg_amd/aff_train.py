"""Stage 3 of the reference's pipeline, aff_train.py, on the MI355X path: the AffinityNet trains here.

    python -m wseg_amd.aff_train --weights <ckpt.pth|procedural> --la_crf_dir DIR --ha_crf_dir DIR ...

The reference's flags and defaults (aff_train.py:15-28; `--network` defaults to this package's module, `--weights procedural` as the other
CLIs have it, `--precision` is the one additive flag).  `--val_list` is parsed and unused, as there.

`AffTrainer(model, optimizer).step(img, label_map)` is the product path: backbone with saved activations -> ELU head -> the pair loss on
the uint8 label map (csrc/aff_loss.hip: forward and gradient) -> head backward -> trunk backward with the conv4 / conv5 gradients as taps
(Engine.run_trunk_backward) -> PolyOptimizer's fused SGD.  No autograd graph and no host synchronisation; it returns the seven scalars of
the reference's AverageMeter (aff_loss.STATS) as one device tensor.  The route through autograd — `Net.affinities_train` with the
reference's own three loss lines as torch ops — computes the same step (tests/test_gpu_aff_train.py).  One process, one GPU: the
data-parallel exchange of the contrast trainer is not wired to this step.
"""
import argparse
import os
import random
import time

import numpy as np
import torch

from . import aff_loss
from . import synth
from .engine import AFF_FEAT_C
from .optim import build_optimizer            # (tests and scripts import it from here)
from .stage_io import load_net

KEYS = aff_loss.STATS
LOG_EVERY = 50


def max_step_of(n_images, batch_size, max_epoches):
    """aff_train.py:70"""
    return n_images // batch_size * max_epoches


class AffTrainer:
    def __init__(self, model, optimizer, capture=False):
        self.model, self.optimizer = model, optimizer
        self.capture, self.last_saved = capture, None     # tests: keep the saved context of the last step (activations stay alive)

    def step(self, img, label_map):
        """One step of aff_train.py:105-123 on img float32 [N, 3, H, W] and label_map uint8 [N, H/8, W/8] (0 background, 1..20 a class,
        255 ignore), both on the device.  Returns the seven scalars [loss, bg_loss, fg_loss, neg_loss, bg_cnt, fg_cnt, neg_cnt] (device)."""
        if not img.is_cuda:
            raise RuntimeError("AffTrainer.step needs GPU tensors (no CPU fallback)")
        model = self.model
        f9, (h, w, r), saved = model.train_forward(img)
        self.last_saved = saved if self.capture else None
        self.optimizer.zero_grad()
        out7, lctx = aff_loss.aff_loss_rows(f9, AFF_FEAT_C, AFF_FEAT_C, label_map, img.shape[0], h, w, r)
        d_f9 = aff_loss.aff_loss_rows_backward(lctx)
        model.train_backward(saved, d_f9)
        self.optimizer.step()
        return out7


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--batch_size", default=8, type=int)
    parser.add_argument("--max_epoches", default=8, type=int)
    parser.add_argument("--network", default="wseg_amd.resnet38_aff", type=str)
    parser.add_argument("--lr", default=0.01, type=float)
    parser.add_argument("--num_workers", default=8, type=int)
    parser.add_argument("--wt_dec", default=5e-4, type=float)
    parser.add_argument("--train_list", default="voc12/train_aug.txt", type=str)
    parser.add_argument("--val_list", default="voc12/val.txt", type=str)
    parser.add_argument("--session_name", default="resnet38", type=str)
    parser.add_argument("--crop_size", default=448, type=int)
    parser.add_argument("--weights", required=True, type=str)
    parser.add_argument("--voc12_root", default='VOC2012', type=str)
    parser.add_argument("--la_crf_dir", required=True, type=str)
    parser.add_argument("--ha_crf_dir", required=True, type=str)
    parser.add_argument("--precision", default=None, choices=[None, "bf16", "fp32", "bf16x3"])
    return parser


def main(argv=None):
    from . import aff_data
    args = make_parser().parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(os.path.join('result', args.session_name), exist_ok=True)
    print(vars(args))

    ds = aff_data.VOC12AffDatasetRaw(args.train_list, args.la_crf_dir, args.ha_crf_dir, args.voc12_root, args.crop_size)
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers, pin_memory=True,
                                         drop_last=True, collate_fn=aff_data.aff_collate,
                                         worker_init_fn=lambda wid: (np.random.seed(1 + wid), random.seed(1 + wid)))
    to_device = aff_data.DeviceAffData(dev, args.crop_size)
    max_step = max_step_of(len(ds), args.batch_size, args.max_epoches)
    model = load_net(args.network, args.weights, args.precision, synth.procedural_aff_state_dict, strict=False, warn_mismatch=True)
    optimizer = build_optimizer(model, args.lr, args.wt_dec, max_step)

    model.cuda(dev)
    model.train()
    trainer = AffTrainer(model, optimizer)

    sums, cnt = torch.zeros(len(KEYS), device=dev), 0
    t_start = stage_start = time.time()
    for ep in range(args.max_epoches):
        for itn, batch in enumerate(loader):
            img, label = to_device(batch)
            sums += trainer.step(img, label)                # device-side accumulation: no per-step host sync
            cnt += 1
            if (optimizer.global_step - 1) % LOG_EVERY == 0:
                elapsed = time.time() - t_start
                est_finish = t_start + elapsed / (optimizer.global_step / max_step)
                avg = (sums / cnt).tolist()                 # the only read-back of scalars
                print('Iter:%5d/%5d' % (optimizer.global_step - 1, max_step),
                      'loss:%.4f %.4f %.4f %.4f' % tuple(avg[:4]),
                      'cnt:%.0f %.0f %.0f' % tuple(avg[4:]),
                      'imps:%.1f' % ((itn + 1) * args.batch_size / (time.time() - stage_start)),
                      'Fin:%s' % time.ctime(int(est_finish)),
                      'lr: %.4f' % (optimizer.param_groups[0]['lr']), flush=True)
                sums.zero_()
                cnt = 0
        print('')
        stage_start = time.time()
    torch.save(model.state_dict(), os.path.join('result', args.session_name, 'aff.pth'))


if __name__ == '__main__':
    main()
