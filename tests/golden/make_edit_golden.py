#!/usr/bin/env python3
"""Generate tests/golden/edit_golden.npz: the reference's edit assembly, EXECUTED from its own source.

textural/edit_vkitti.py and textural/edit_benchmark.py are scripts that cannot run as a whole here (option classes with
module-level side effects, `dominate`, checkpoints).  This script takes with `ast`, from where they lie,
  * edit_vkitti.py:41-54    the set-up of the source frame (label + 1, instance ids * 1000, cars without an instance -> misc)
  * edit_vkitti.py:63-103   the body of the edit loop up to, not including, the fake_inference call
  * edit_benchmark.py:66-78 and :83-126, the same two pieces of the benchmark script (one source per edited frame; an
    instance without a source code is skipped instead of raising)
and executes them on seeded frames: `Image.open` reads temporary PNG / JSON files written here, `get_params` /
`get_transform` are the reference's own data/base_dataset.py on the torchvision stub of make_loader_golden.py (torchvision
0.2.1's published behaviour on the real Pillow), `feat_dict` -- the encoder's product, edit_vkitti.py:57 -- is a seeded
table with one code per instance id of the source frame.
The fixture stores the frames' source arrays, the code table and what the blocks left in `segm`, `inst`, `pose`, `feat`,
`normal`; tests/test_gpu_edit.py holds data.assemble.assemble_edit against it bit for bit.  The edit_vkitti cases are
chosen without a missing id (the reference raises KeyError there; checked below).  Runs only where the reference exists.
"""
import ast
import json
import os
import shutil
import sys
import tempfile
import types
from math import pi

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = os.environ.get('SDN_REFERENCE_ROOT', '/root/reference')
H, W = 46, 158          # resize_or_crop 'none' with n_downsample_global 3: make_power_2 -> 48 x 160 through NEAREST / BICUBIC
FEAT_NUM = 3


def block(path, first, last, inside_for=True, opens=None):
    """the top-level (or loop-body) statements of `path` lying in lines first..last, compiled"""
    src = open(path).read()
    tree = ast.parse(src)
    body = tree.body
    if inside_for:
        loops = [st for st in tree.body if isinstance(st, ast.For) and st.lineno < first and st.end_lineno >= last]
        assert len(loops) == 1, path
        body = loops[0].body
    sts = [st for st in body if first <= st.lineno and st.end_lineno <= last]
    assert sts and sts[0].lineno == first and sts[-1].end_lineno == last, (path, sts[0].lineno, sts[-1].end_lineno)
    if opens is not None:
        assert ast.get_source_segment(src, sts[0]).startswith(opens), ast.get_source_segment(src, sts[0])
    return compile(ast.Module(body=sts, type_ignores=[]), path, 'exec')


def blocky(rng, cell=6):
    """an RGB map of random 6 x 6 cells: edges for the BICUBIC resize, and it still compresses"""
    a = rng.integers(0, 256, ((H + cell - 1) // cell, (W + cell - 1) // cell, 3), dtype=np.uint8)
    return np.ascontiguousarray(a.repeat(cell, 0).repeat(cell, 1)[:H, :W])


def source_frame(rng):
    """label map (raw ids 0..12; 1 = car, 11 = van before the + 1), image, instance map with three objects; some car pixels
    carry no instance, raw label 4 (-> "misc" 5) and 8 (-> 9) exist without an instance"""
    segm = np.zeros((H, W), np.uint8)
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 16):
            segm[y0:y0 + 8, x0:x0 + 16] = rng.choice([0, 3, 4, 5, 6, 8, 9])
    segm[0:6, 0:12] = 4
    segm[40:46, 0:12] = 8
    inst = np.zeros((H, W), np.uint8)
    boxes = {1: (10, 10, 14, 30, 1), 2: (20, 60, 16, 36, 11), 3: (8, 110, 10, 24, 1)}     # y, x, h, w, raw label
    for k, (y, x, h, w, lab) in boxes.items():
        inst[y:y + h, x:x + w] = k
        segm[y - 2:y + h + 2, x - 3:x + w + 3] = lab          # a rim of car pixels without an instance
    image = blocky(rng)
    return segm, image, inst, boxes


def edited_frame(rng, boxes, moves, extra=None):
    """objects re-painted at (dy, dx) offsets; `moves` {id: (dy, dx, class_id)}; extra {id: (y, x, h, w, class_id | None)}"""
    inst = np.zeros((H, W), np.uint8)
    js = {}
    for k, (dy, dx, cls) in moves.items():
        y, x, h, w, _ = boxes[k]
        inst[y + dy:y + dy + h, x + dx:x + dx + w] = k
        js[str(k)] = {'class_id': cls, 'depth': float(rng.uniform(5, 40)), 'alpha': float(rng.uniform(-pi, pi))}
    for k, (y, x, h, w, cls) in (extra or {}).items():
        inst[y:y + h, x:x + w] = k
        if cls is not None:
            js[str(k)] = {'class_id': cls, 'depth': 9.0, 'alpha': float(rng.uniform(-pi, pi))}
    return inst, js, blocky(rng)


def save(path, arr, mode):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    PIL.Image.fromarray(arr, mode).save(path)


def options(tmp, bins):
    return types.SimpleNamespace(resize_or_crop='none', loadSize=160, fineWidth=160, fineHeight=48, isTrain=False, no_flip=True,
                                 n_downsample_global=3, netG='global', n_local_enhancers=0, feat_num=FEAT_NUM,
                                 feat_pose_num_bins=bins, feat_normal=os.path.join(tmp, 'edit'), edit_dir=os.path.join(tmp, 'edit'),
                                 segm_precomputed_path=os.path.join(tmp, 'segm'), dataroot=os.path.join(tmp, 'root'))


def namespace(opt, get_params, get_transform):
    return {'torch': torch, 'np': np, 'os': os, 'json': json, 'pi': pi, 'Image': PIL.Image, 'opt': opt, 'get_params': get_params,
            'get_transform': get_transform, 'print': lambda *a, **k: None,
            'bins': (np.array(list(range(-180, 181, 360 // opt.feat_pose_num_bins))) / 180) if opt.feat_pose_num_bins else None}


def code_table(rng, ids):
    codes = rng.uniform(-1, 1, (len(ids), FEAT_NUM)).astype(np.float32)
    return codes, {int(i): [float(v) for v in row] for i, row in zip(ids, codes)}


def store(out, p, ns, frame_no):
    q = '%sf%d/' % (p, frame_no)
    for k in ('segm', 'inst', 'pose', 'feat', 'normal'):
        out[q + k] = ns[k].numpy().astype(np.float32)
        assert np.array_equal(out[q + k], ns[k].numpy()), k       # ids <= 255000: exact in fp32


def main():
    from make_loader_golden import torchvision_stub
    tv, tr = torchvision_stub()
    sys.modules['torchvision'] = tv
    sys.modules['torchvision.transforms'] = tr
    sys.path.insert(0, os.path.join(REF, 'textural'))
    from data.base_dataset import get_params, get_transform        # the reference module, as it lies
    torch.Tensor.cuda = lambda self, *a, **k: self
    vk = os.path.join(REF, 'textural', 'edit_vkitti.py')
    bm = os.path.join(REF, 'textural', 'edit_benchmark.py')
    vk_setup = block(vk, 41, 54, inside_for=False, opens='base_img = Image.open(opt.edit_source)')
    vk_body = block(vk, 63, 103, opens='inst = Image.open(')
    bm_setup = block(bm, 66, 78, opens='params = get_params(')
    bm_body = block(bm, 83, 126, opens='inst = Image.open(')
    out = {}
    names = []
    # ---- edit_vkitti: one source, several edited frames; 24 pose bins and feat_pose_num_bins = 0
    for name, bins, seed in (('vkitti24', 24, 5), ('vkitti0', 0, 6)):
        rng = np.random.default_rng(seed)
        tmp = tempfile.mkdtemp(prefix='edit_golden_')
        try:
            opt = options(tmp, bins)
            segm, image, inst0, boxes = source_frame(rng)
            frames = [edited_frame(rng, boxes, {1: (0, 0, 1), 2: (0, 0, 2), 3: (0, 0, 1)}),
                      # object 2 (a van) moved onto former misc, former road and part of object 1's former car pixels
                      edited_frame(rng, boxes, {1: (1, -4, 1), 2: (-8, -28, 2)}),
                      (np.zeros((H, W), np.uint8), {}, None)]        # no objects: empty JSON, no normal file
            opt.edit_source = os.path.join(tmp, 'root', 'source.png')
            save(opt.edit_source, image, 'RGB')
            opt.segm_precomputed_path = os.path.join(tmp, 'segm', 'source.png')
            save(opt.segm_precomputed_path, segm, 'L')
            for i, (ei, js, nrm) in enumerate(frames):
                save(os.path.join(opt.edit_dir, '%05d.png' % i), inst0 if i == 0 else ei, 'L')
                if i == 0:
                    frames[0] = (inst0, js, nrm)
                with open(os.path.join(opt.edit_dir, '%05d.json' % i), 'w') as f:
                    json.dump(js, f)
                if nrm is not None:
                    save(os.path.join(opt.edit_dir, '%05d-normal.png' % i), nrm, 'RGB')
            ns = namespace(opt, get_params, get_transform)
            exec(vk_setup, ns)
            ids = np.unique(ns['base_inst'].numpy().astype(int))
            codes, ns['feat_dict'] = code_table(rng, ids)
            p = name + '/'
            out[p + 'cfg'] = np.asarray(json.dumps({'feat_pose_num_bins': bins, 'per_frame_source': False, 'frames': len(frames)}))
            out[p + 's0/segm'], out[p + 's0/image'], out[p + 's0/inst'] = segm, image, inst0
            out[p + 's0/base_segm'] = ns['base_segm'].numpy()
            out[p + 's0/base_inst'] = ns['base_inst'].numpy()
            out[p + 's0/crop_pos'] = np.asarray(ns['params']['crop_pos'], np.int64)
            out[p + 'code_ids'], out[p + 'codes'] = ids.astype(np.int64), codes
            for i, (ei, js, nrm) in enumerate(frames):
                ns['i'] = i
                exec(vk_body, ns)          # a missing id raises KeyError here, as in the reference
                assert set(np.unique(ns['inst'].numpy()).tolist()) <= set(ids.tolist())
                q = '%sf%d/' % (p, i)
                out[q + 'edit_inst'], out[q + 'json'] = ei, np.asarray(json.dumps(js, sort_keys=True))
                if nrm is not None:
                    out[q + 'edit_normal'] = nrm
                store(out, p, ns, i)
                moved = ns['inst'].numpy()[0]
                print(name, 'frame', i, 'ids', np.unique(moved).tolist(), 'labels', np.unique(ns['segm'].numpy()).tolist(),
                      'pose', np.unique(ns['pose'].numpy()).tolist())
            names.append(name)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    # ---- edit_benchmark: one source per edited frame, one shared code table; object 7 has no source code, raw id 9 is not
    # in the JSON (the block leaves it: it reads the code of LABEL 9)
    name, bins = 'bench24', 24
    rng = np.random.default_rng(7)
    tmp = tempfile.mkdtemp(prefix='edit_golden_')
    try:
        opt = options(tmp, bins)
        p = name + '/'
        pairs = []
        all_ids = set()
        for i in range(3):
            segm, image, inst0, boxes = source_frame(rng)
            moves = [{1: (2, 6, 1), 2: (0, -10, 2), 3: (0, 0, 1)}, {1: (0, 0, 2), 3: (4, -20, 1)}, {2: (-6, 14, 2)}][i]
            extra = [{7: (30, 130, 8, 20, 1)}, {9: (34, 20, 6, 14, None)}, None][i]
            ei, js, nrm = edited_frame(rng, boxes, moves, extra)
            edit_source, edit_target = 'w%d/clone/src.png' % i, 'w%d/clone/dst.png' % i
            save(os.path.join(opt.segm_precomputed_path, edit_source), segm, 'L')
            save(os.path.join(opt.edit_dir, edit_source), inst0, 'L')
            save(os.path.join(opt.edit_dir, edit_target), ei, 'L')
            with open(os.path.join(opt.edit_dir, edit_target.replace('.png', '.json')), 'w') as f:
                json.dump(js, f)
            if i != 2:
                save(os.path.join(opt.edit_dir, edit_target.replace('.png', '-normal.png')), nrm, 'RGB')
            ns = namespace(opt, get_params, get_transform)
            ns.update(base_segm=PIL.Image.open(os.path.join(opt.segm_precomputed_path, edit_source)),
                      base_inst=PIL.Image.open(os.path.join(opt.edit_dir, edit_source)), base_inst_exist=1,
                      base_img=PIL.Image.fromarray(image, 'RGB'), target_img=PIL.Image.fromarray(image, 'RGB'),
                      edit_source=edit_source, edit_target=edit_target)
            exec(bm_setup, ns)
            all_ids |= set(np.unique(ns['base_inst'].numpy().astype(int)).tolist())
            pairs.append((ns, segm, image, inst0, ei, js, nrm if i != 2 else None))
        ids = np.asarray(sorted(all_ids), np.int64)
        assert 7000 not in all_ids and 9 in all_ids
        codes, feat_dict = code_table(rng, ids)
        out[p + 'cfg'] = np.asarray(json.dumps({'feat_pose_num_bins': bins, 'per_frame_source': True, 'frames': len(pairs)}))
        out[p + 'code_ids'], out[p + 'codes'] = ids, codes
        for i, (ns, segm, image, inst0, ei, js, nrm) in enumerate(pairs):
            ns['feat_dict'] = feat_dict
            exec(bm_body, ns)
            s = '%ss%d/' % (p, i)
            out[s + 'segm'], out[s + 'image'], out[s + 'inst'] = segm, image, inst0
            out[s + 'base_segm'], out[s + 'base_inst'] = ns['base_segm'].numpy(), ns['base_inst'].numpy()
            out[s + 'crop_pos'] = np.asarray(ns['params']['crop_pos'], np.int64)
            q = '%sf%d/' % (p, i)
            out[q + 'edit_inst'], out[q + 'json'] = ei, np.asarray(json.dumps(js, sort_keys=True))
            if nrm is not None:
                out[q + 'edit_normal'] = nrm
            store(out, p, ns, i)
            final = ns['inst'].numpy().astype(int)
            lost = int(sum((final == v).sum() for v in np.unique(final) if int(v) not in feat_dict))
            out[q + 'missing'] = np.int64(lost)
            print(name, 'pair', i, 'ids', np.unique(final).tolist(), 'pixels without a code', lost)
        assert int(out[p + 'f0/missing']) > 0 and int(out[p + 'f1/missing']) == 0
        names.append(name)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out['cases'] = np.asarray(json.dumps(names))
    path = os.path.join(HERE, 'edit_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path))


if __name__ == '__main__':
    main()
