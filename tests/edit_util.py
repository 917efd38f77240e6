"""Shared by tests/test_edit_assemble.py and tests/test_gpu_edit.py: the fixture tests/golden/edit_golden.npz (written by
tests/golden/make_edit_golden.py from the reference's own edit scripts) and the options its frames were made with."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edit_golden.npz')
PARAMS = {'crop_pos': (0, 0), 'flip': False}
E2E_GATE = 2e-5   # tests/test_gpu_pipeline_e2e.py:150-152: batched against per-frame fake_inference, relative L2


def options(bins, **over):
    """the fixture's option set on top of the model's defaults (46 x 158 frames -> 48 x 160 through make_power_2)"""
    from models.pix2pixHD_model import default_options
    kw = dict(gpu_ids=[0], batchSize=1, resize_or_crop='none', loadSize=160, fineWidth=160, fineHeight=48, isTrain=True,
              no_flip=True, n_downsample_global=3, netG='global', n_local_enhancers=0, feat_num=3, feat_pose='1',
              feat_pose_num_bins=bins, feat_normal='1', segm_precomputed_path='geometric', inst_precomputed_path='geometric',
              no_vgg_loss=True, num_D=2, ngf=8, n_blocks_global=2, ndf=8, nef=4, n_downsample_E=2)
    kw.update(over)
    return default_options(**kw)


def chw(a, dev=None):
    """[H, W] or [H, W, C] uint8 array -> uint8 [C, H, W] tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[:, :, None])).permute(2, 0, 1).contiguous()
    return t if dev is None else t.to(dev)


class Case:
    def __init__(self, z, name):
        self.z, self.name = z, name
        self.cfg = json.loads(str(z[name + '/cfg']))
        self.bins = self.cfg['feat_pose_num_bins']
        self.per_frame_source = self.cfg['per_frame_source']
        self.frames = self.cfg['frames']
        self.code_ids = z[name + '/code_ids']
        self.codes = z[name + '/codes']

    def source(self, i):
        """(segm, image, inst uint8 arrays, expected base label, expected base inst) of frame i's source"""
        s = '%s/s%d/' % (self.name, i if self.per_frame_source else 0)
        return tuple(self.z[s + k] for k in ('segm', 'image', 'inst', 'base_segm', 'base_inst'))

    def edit(self, i):
        """(edit inst uint8 [H, W], JSON dict, normal uint8 [H, W, 3] or None)"""
        q = '%s/f%d/' % (self.name, i)
        nrm = self.z[q + 'edit_normal'] if q + 'edit_normal' in self.z.files else None
        return self.z[q + 'edit_inst'], json.loads(str(self.z[q + 'json'])), nrm

    def expected(self, i):
        q = '%s/f%d/' % (self.name, i)
        return {k: self.z[q + k] for k in ('segm', 'inst', 'pose', 'feat', 'normal')}

    def missing(self, i):
        q = '%s/f%d/missing' % (self.name, i)
        return int(self.z[q]) if q in self.z.files else 0


def cases():
    z = np.load(GOLD)
    return [Case(z, n) for n in json.loads(str(z['cases']))]
