#!/usr/bin/env python3
"""CLI entry point (parity with reference `main.py`).

    python main.py --phase=train
    python main.py --phase=eval --model_file='./models/xxxxxx.npy' [--beam_size=3]
    python main.py --phase=test --model_file='./models/xxxxxx.npy' [--beam_size=3]

Same seven flags as reference main.py:15-36 (+ MI355X extras: --device,
--synthetic, --compute_dtype, --fused_beam, --eval_batch_size,
--loader_threads, --device_image_prep).
Dispatches to train/eval/test on the runtime (sat_amd.models.BaseModel), loading checkpoints / pretrained CNNs
exactly like reference main.py:49-72.
"""

import argparse

import torch

from config import Config
from sat_amd.data.dataset import (prepare_eval_data, prepare_test_data,
                                  prepare_train_data)
from sat_amd.models.base_model import BaseModel


def build_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--phase', default='train',
                   choices=['train', 'eval', 'test'],
                   help='The phase can be train, eval or test')
    p.add_argument('--load', action='store_true',
                   help='Turn on to load a pretrained model from either '
                        'the latest checkpoint or a specified file')
    p.add_argument('--model_file', default=None,
                   help='If sepcified, load a pretrained model from this '
                        'file')
    p.add_argument('--load_cnn', action='store_true',
                   help='Turn on to load a pretrained CNN model')
    p.add_argument('--cnn_model_file', default='./vgg16_no_fc.npy',
                   help='The file containing a pretrained CNN model')
    p.add_argument('--train_cnn', action='store_true',
                   help='Turn on to train both CNN and RNN. Otherwise, '
                        'only RNN is trained')
    p.add_argument('--beam_size', type=int, default=3,
                   help='The size of beam search for caption generation')
    # MI355X-native extras
    p.add_argument('--device', default='auto',
                   choices=['auto', 'cuda', 'cpu'])
    p.add_argument('--synthetic', action='store_true',
                   help='Use synthetic COCO-shaped data (no files/network)')
    p.add_argument('--compute_dtype', default=None,
                   choices=['bf16', 'fp32'])
    p.add_argument('--fused_beam', action='store_true',
                   help='Beam search through the fused, graph-captured '
                        'inference engine (config.use_fused_beam)')
    p.add_argument('--eval_batch_size', type=int, default=1,
                   help='Images per beam-search batch in the eval phase '
                        '(the reference forces 1)')
    p.add_argument('--loader_threads', type=int, default=0,
                   help='Decode the coming batches\' image files on this '
                        'many threads (config.num_loader_threads; 0 = '
                        'load each batch when it is needed)')
    p.add_argument('--device_image_prep', action='store_true',
                   help='Resize and normalise images on the device '
                        '(config.device_image_prep)')
    return p


def build_config(args):
    """Config for the parsed flags."""
    config = Config()
    config.phase = args.phase
    config.train_cnn = args.train_cnn
    config.beam_size = args.beam_size
    config.device = args.device
    if args.synthetic:
        config.synthetic_data = True
    if args.compute_dtype:
        config.compute_dtype = args.compute_dtype
    if args.fused_beam:
        config.use_fused_beam = True
    if args.loader_threads:
        config.num_loader_threads = args.loader_threads
    if args.device_image_prep:
        config.device_image_prep = True
    if args.phase == 'eval':
        # reference main.py:59 forces eval batch 1 (the default here)
        config.batch_size = args.eval_batch_size
    return config


def main(argv=None):
    args = build_parser().parse_args(argv)
    config = build_config(args)

    torch.manual_seed(config.seed)

    if args.phase == 'train':
        data = prepare_train_data(config)
        model = BaseModel(config)
        if args.load:
            model.load(args.model_file)
        if args.load_cnn:
            model.load_cnn(args.cnn_model_file)
        model.train(data)

    elif args.phase == 'eval':
        coco, data, vocabulary = prepare_eval_data(config)
        model = BaseModel(config)
        model.load(args.model_file)
        model.eval(coco, data, vocabulary)

    else:
        data, vocabulary = prepare_test_data(config)
        model = BaseModel(config)
        model.load(args.model_file)
        model.test(data, vocabulary)


if __name__ == '__main__':
    main()
