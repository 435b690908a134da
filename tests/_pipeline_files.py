"""Image files and a small file-backed corpus for the input-pipeline
tests, written with PIL into a directory the test owns."""

import json
import os

import numpy as np
from PIL import Image

CAPS = ['a red dog sitting on a table.', 'a small cat on a beach.',
        'a young man riding a horse.', 'a large bus on a street.',
        'a white bird on a bench.', 'a black boat near a field.']


def smooth_image(h, w, seed):
    """A uint8 [h,w,3] image with structure at every scale (JPEG keeps
    it, unlike noise)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.01, 0.3, 3)
        img[:, :, c] = 127 + 100 * np.sin(fy * yy + ph) * np.cos(fx * xx)
    img += rng.uniform(-20, 20, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def write_images(root, sizes, ext='jpg', seed=0):
    """One file per (H, W) -> list of paths."""
    os.makedirs(root, exist_ok=True)
    files = []
    for i, (h, w) in enumerate(sizes):
        f = os.path.join(root, 'im_%03d_%dx%d.%s' % (i, h, w, ext))
        Image.fromarray(smooth_image(h, w, seed + i)).save(f)
        files.append(f)
    return files


def write_corpus(root, sizes, prefix, start_id=1):
    """Images + a COCO captions file -> (image dir, captions file)."""
    img_dir = os.path.join(root, 'images')
    os.makedirs(img_dir, exist_ok=True)
    images, anns = [], []
    for i, (h, w) in enumerate(sizes):
        iid = start_id + i
        name = '%s_%06d.jpg' % (prefix, iid)
        Image.fromarray(smooth_image(h, w, iid)).save(
            os.path.join(img_dir, name))
        images.append({'id': iid, 'file_name': name})
        anns.append({'id': iid, 'image_id': iid,
                     'caption': CAPS[i % len(CAPS)]})
    caps_file = os.path.join(root, 'captions.json')
    with open(caps_file, 'w') as f:
        json.dump({'images': images, 'annotations': anns}, f)
    return img_dir, caps_file


def file_config(cfg, tmp_path, train_sizes, val_sizes):
    """Point a tiny_config at a fresh file-backed corpus."""
    cfg.synthetic_data = False
    cfg.vocabulary_size = 100
    train_dir, train_caps = write_corpus(
        str(tmp_path / 'train'), train_sizes, 'tr')
    val_dir, val_caps = write_corpus(
        str(tmp_path / 'val'), val_sizes, 'va', start_id=100)
    cfg.train_image_dir = train_dir
    cfg.train_caption_file = train_caps
    cfg.eval_image_dir = val_dir
    cfg.eval_caption_file = val_caps
    cfg.temp_annotation_file = str(tmp_path / 'anns.csv')
    cfg.temp_data_file = str(tmp_path / 'data.npy')
    cfg.vocabulary_file = str(tmp_path / 'vocabulary.csv')
    cfg.max_train_ann_num = len(train_sizes)
    cfg.max_eval_ann_num = len(val_sizes)
    return cfg


class Recorder(object):
    """Wraps model.compute_contexts and keeps a copy of every image
    tensor that reaches it."""

    def __init__(self, caption_generator):
        self.images = []
        inner = caption_generator.compute_contexts

        def compute_contexts(images):
            self.images.append(images.detach().clone())
            return inner(images)
        caption_generator.compute_contexts = compute_contexts
