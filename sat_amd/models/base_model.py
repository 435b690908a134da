"""BaseModel — the runtime layer (parity with reference `base_model.py`).

Owns the CaptionGenerator, the image loader, the optimizer, global_step and
summaries; implements the epoch/batch training loop (base_model.py:39-68),
COCO evaluation with beam search + metric scoring (:70-117), arbitrary-image
testing with overlay artifacts (:119-161), batched beam search (:163-240)
and `.npy`-dict checkpointing (:242-297).

MI355X-native differences from the reference runtime:
  * beam search keeps LSTM state device-resident and expands ALL live
    hypotheses of a batch in ONE decode_step launch per step, instead of the
    reference's beam_size sess.run round-trips with host-side state ferrying
    (base_model.py:191-212).  Candidate scoring/ordering semantics are kept
    bit-for-bit: beam_size+1 expansion, '.'-termination, probability-product
    scores, per-image bounded TopN heaps.  The reference's
    `list(set(batch))` image-reorder bug (base_model.py:83) is deliberately
    NOT reproduced.
  * under torch.distributed (RCCL over xGMI), gradient all-reduce runs in
    bucketed overlap with backward (sat_amd.parallel); rank 0 is chief for
    checkpoints/summaries, mirroring is_chief (main_distributed.py:64).
"""

import json
import os

import numpy as np
import pandas as pd
import torch
from tqdm import tqdm

from ..data.image_loader import ImageLoader
from ..data.synthetic import SyntheticImageLoader
from ..evalcap.eval import COCOEvalCap
from ..optim import Optimizer
from ..utils import checkpoint as ckpt
from ..utils.summary import SummaryWriter
from ..utils.topn import CaptionData, TopN
from .caption_generator import CaptionGenerator


def _resolve_device(config):
    want = getattr(config, 'device', 'auto')
    if want == 'cpu':
        return torch.device('cpu')
    if want == 'cuda' or (want == 'auto' and torch.cuda.is_available()):
        return torch.device('cuda')
    return torch.device('cpu')


class BaseModel(object):
    def __init__(self, config):
        self.config = config
        self.device = _resolve_device(config)
        self.image_shape = [224, 224, 3]
        if getattr(config, 'synthetic_data', False):
            self.image_loader = SyntheticImageLoader(
                self.image_shape, getattr(config, 'seed', 0),
                getattr(config, 'synthetic_mode', 'noise'))
        else:
            self.image_loader = ImageLoader(None, self.image_shape)

        self.model = CaptionGenerator(config).to(self.device)
        self.global_step = 0
        self._engine = None
        self._prep = None               # ImagePrep, made on first use
        self._staged = None             # (files, images) loaded ahead

        self.is_train = getattr(config, 'phase', 'train') == 'train'
        self.optimizer = Optimizer(
            config, self.model.parameters()) if self.is_train else None

        # bf16 shadow weights: the fused Adam refreshes persistent bf16
        # copies of the BPTT weights in its update pass, removing the
        # per-forward weight casts and cast-node backwards from the
        # training step (sat_amd/optim.py, models/decoder.py)
        if (self.optimizer is not None and self.device.type == 'cuda'
                and getattr(config, 'use_hip_kernels', True)
                and getattr(config, 'use_bptt', True)):
            smap = self.model.decoder.ensure_shadows()
            if smap:
                self.optimizer.register_shadows(smap)
                self.model.decoder._shadows_active = True

        # distributed (one process per GPU over RCCL; gloo on CPU)
        self.ddp = None
        if torch.distributed.is_available() \
                and torch.distributed.is_initialized():
            from ..parallel.ddp import DataParallelGrads
            self.ddp = DataParallelGrads(
                self.model,
                bucket_mb=getattr(config, 'allreduce_bucket_mb', 16))
        self.rank = (torch.distributed.get_rank()
                     if self.ddp is not None else 0)
        self.is_chief = self.rank == 0

    # ------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------

    def _images_to_device(self, images_np):
        """[N,H,W,3] float32 numpy -> [N,3,H,W] torch on device."""
        t = torch.from_numpy(np.ascontiguousarray(images_np))
        t = t.permute(0, 3, 1, 2).contiguous()
        return t.to(self.device, non_blocking=True)

    # ---- input pipeline (sat_amd/data/pipeline.py; off by default) ----

    def _image_prep(self):
        """The ImagePrep behind config.device_image_prep, or None: it
        needs decoded uint8 images (not the synthetic loader) and a
        per-channel mean."""
        if not getattr(self.config, 'device_image_prep', False) \
                or type(self.image_loader) is not ImageLoader \
                or np.shape(self.image_loader.mean) != (3,):
            return None
        if self._prep is None:
            from ..data.pipeline import ImagePrep
            bf16 = self.device.type == 'cuda' and getattr(
                self.config, 'compute_dtype', 'bf16') == 'bf16'
            self._prep = ImagePrep(
                self.image_loader.mean, self.image_loader.image_shape,
                self.device, torch.bfloat16 if bf16 else torch.float32)
        return self._prep

    def _load_batch(self, image_files):
        """Files -> the [N,3,H,W] image tensor on the device: what
        `_batches` loaded ahead for exactly this batch, else loaded here,
        through ImagePrep with config.device_image_prep."""
        staged, self._staged = self._staged, None
        if staged is not None and staged[0] is image_files:
            images = staged[1]
        elif self._image_prep() is not None:
            from ..data.pipeline import decode_u8
            images = self._image_prep()([decode_u8(f) for f in image_files])
        else:
            images = self.image_loader.load_images(image_files)
        if isinstance(images, np.ndarray):
            images = self._images_to_device(images)
        if not images.is_cuda:
            # the CPU encoder runs in the layout it is handed, and its
            # sums differ in the last bits between layouts: keep NCHW
            images = images.contiguous()
        return images

    def _batches(self, data):
        """One epoch of `data.next_batch()` results.  With
        config.num_loader_threads > 0 a BatchPrefetcher loads the images
        of the coming batches on worker threads, and `_load_batch` of a
        yielded batch's files returns them."""
        threads = getattr(self.config, 'num_loader_threads', 0)
        if threads <= 0:
            for _ in range(data.num_batches):
                yield data.next_batch()
            return
        from ..data.pipeline import BatchPrefetcher
        prefetcher = BatchPrefetcher(
            data, self.image_loader, self._image_prep(), threads,
            getattr(self.config, 'prefetch_batches', 2))
        try:
            for batch, images in prefetcher:
                self._staged = (batch[0] if data.is_train else batch,
                                images)
                yield batch
        finally:
            prefetcher.close()

    def train_step(self, images, sentences, masks):
        """One fwd+bwd+optimizer step on device tensors. Returns loss dict.

        On GPU with config.use_hip_graph the whole step runs as one hipGraph
        replay (sat_amd.engine.GraphedTrainStep)."""
        self.model.train()
        if self._engine is None and self.device.type == 'cuda' \
                and getattr(self.config, 'use_hip_graph', True):
            from ..engine import GraphedTrainStep
            self._engine = GraphedTrainStep(self.model, self.optimizer,
                                            self.ddp)
        if self._engine is not None:
            out = self._engine.step(images, sentences, masks)
        else:
            out = self.model(images, sentences, masks)
            self.optimizer.zero_grad()
            out['total_loss'].backward()
            if self.ddp is not None:
                self.ddp.finish_backward()
            self.optimizer.step()
        self.global_step += 1
        return out

    def train(self, train_data):
        """Epoch/batch training loop (reference base_model.py:39-68)."""
        config = self.config
        os.makedirs(config.summary_dir, exist_ok=True)
        writer = SummaryWriter(config.summary_dir) if self.is_chief else None

        for _ in tqdm(range(config.num_epochs), desc='epoch'):
            for image_files, sentences, masks in tqdm(
                    self._batches(train_data), total=train_data.num_batches,
                    desc='batch', leave=False):
                images = self._load_batch(image_files)
                sentences = torch.as_tensor(
                    sentences, dtype=torch.int64).to(self.device)
                masks = torch.as_tensor(
                    masks, dtype=torch.float32).to(self.device)

                out = self.train_step(images, sentences, masks)

                if (self.global_step + 1) % config.save_period == 0 \
                        and self.is_chief:
                    self.save()
                    if writer is not None:
                        # per-variable mean/std/max/min stats (reference
                        # model.py:534-542 logs these per step; we log at
                        # checkpoint cadence)
                        for name, prm in \
                                self.model.named_parameters():
                            if prm.requires_grad:
                                writer.variable_summary(
                                    name, prm, self.global_step)
                if writer is not None:
                    writer.add_scalars(
                        {k: v.item() for k, v in out.items()
                         if v.numel() == 1}, self.global_step)
            train_data.reset()

        if self.is_chief:
            self.save()
        if writer is not None:
            writer.close()
        print("Training complete.")

    # ------------------------------------------------------------------
    # evaluation
    # ------------------------------------------------------------------

    def eval(self, eval_gt_coco, eval_data, vocabulary):
        """COCO-val evaluation: beam search + metric suite
        (reference base_model.py:70-117)."""
        config = self.config
        os.makedirs(config.eval_result_dir, exist_ok=True)
        results = []
        idx = 0
        for k, batch in enumerate(tqdm(
                self._batches(eval_data), total=eval_data.num_batches,
                desc='batch')):
            caption_data = self.beam_search(batch, vocabulary)

            fake_cnt = 0 if k < eval_data.num_batches - 1 \
                else eval_data.fake_count
            for l in range(eval_data.batch_size - fake_cnt):
                word_idxs = caption_data[l][0].sentence
                caption = vocabulary.get_sentence(word_idxs)
                results.append({
                    'image_id': int(eval_data.image_ids[idx]),
                    'caption': caption})
                idx += 1
                if config.save_eval_result_as_image:
                    self._save_overlay(batch[l], caption,
                                       config.eval_result_dir)

        with open(config.eval_result_file, 'w') as fp:
            json.dump(results, fp)

        eval_result_coco = eval_gt_coco.loadRes(config.eval_result_file)
        scorer = COCOEvalCap(eval_gt_coco, eval_result_coco, eval_data)
        scorer.evaluate()
        print("Evaluation complete.")
        return scorer.eval

    def test(self, test_data, vocabulary):
        """Caption arbitrary images (reference base_model.py:119-161)."""
        config = self.config
        os.makedirs(config.test_result_dir, exist_ok=True)
        captions, scores = [], []
        for k, batch in enumerate(tqdm(
                self._batches(test_data), total=test_data.num_batches,
                desc='path')):
            caption_data = self.beam_search(batch, vocabulary)
            fake_cnt = 0 if k < test_data.num_batches - 1 \
                else test_data.fake_count
            for l in range(test_data.batch_size - fake_cnt):
                word_idxs = caption_data[l][0].sentence
                score = caption_data[l][0].score
                caption = vocabulary.get_sentence(word_idxs)
                captions.append(caption)
                scores.append(score)
                self._save_overlay(batch[l], caption,
                                   config.test_result_dir)

        results = pd.DataFrame({
            'image_files': test_data.image_files[:len(captions)],
            'caption': captions,
            'prob': scores})
        results.to_csv(config.test_result_file)
        print("Testing complete.")
        return results

    def _save_overlay(self, image_file, caption, out_dir):
        """Caption-overlaid image artifact (reference base_model.py:97-107)."""
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
            if str(image_file).startswith('synthetic://'):
                img = self.image_loader.load_image(image_file)
                img = (img - img.min()) / max(float(np.ptp(img)), 1e-6)
            else:
                img = plt.imread(image_file)
            plt.figure()
            plt.imshow(img)
            plt.axis('off')
            plt.title(caption)
            name = os.path.basename(str(image_file)).replace('/', '_') \
                .replace(':', '_')
            plt.savefig(os.path.join(out_dir, name + '_result.jpg'))
            plt.close()
        except Exception as e:  # artifact rendering must never kill a run
            print('overlay skipped: %r' % (e,))

    # ------------------------------------------------------------------
    # beam search (device-resident state)
    # ------------------------------------------------------------------

    @torch.no_grad()
    def beam_search(self, image_files, vocabulary):
        """Beam-search captions for a batch of images
        (semantics of reference base_model.py:163-240).

        Dispatches to the device-resident scorer (one host sync per
        batch) unless config.use_device_beam is False; the host-heap
        path below is the semantics reference.  With
        config.use_fused_beam the fused, graph-captured engine
        (sat_amd/beam.py) takes every batch its GPU form covers."""
        if getattr(self.config, 'use_fused_beam', False) \
                and self._fused_beam_mode() == 'hip':
            return self.beam_search_fused(image_files, vocabulary)
        if getattr(self.config, 'use_device_beam', True):
            return self.beam_search_device(image_files, vocabulary)
        return self.beam_search_host(image_files, vocabulary)

    def _fused_beam_mode(self):
        """What FusedBeamDecoder offers this model: 'hip' (the GPU
        engine), 'twin' (its CPU form) or None (not covered)."""
        if getattr(self, '_fused_beam', None) is None:
            from ..beam import FusedBeamDecoder
            self._fused_beam = FusedBeamDecoder(self.model)
        is_cuda = self.device.type == 'cuda'
        bf16 = is_cuda and getattr(self.config, 'compute_dtype',
                                   'bf16') == 'bf16'
        return self._fused_beam.mode(
            is_cuda, torch.bfloat16 if bf16 else torch.float32,
            getattr(self.config, 'beam_size', 3))

    @torch.no_grad()
    def beam_search_fused(self, image_files, vocabulary):
        """Beam search through sat_amd.beam.FusedBeamDecoder: per-image
        work once, the T steps as fused kernels in one captured graph
        (CPU: the same structure through the op layer's PyTorch twins).
        Covers the 1- and 2-layer decode MLP and, on the GPU, the 1- and
        2-layer attention: the 2-layer attention is hoisted out of the
        loop, the 1-layer one runs inside it as the beam-shared
        `beam_attend` kernel.  Same hypothesis semantics and result
        structure as beam_search_device, which also serves every
        configuration the engine does not cover (on the CPU that includes
        the 1-layer attention)."""
        if self._fused_beam_mode() is None:
            return self.beam_search_device(image_files, vocabulary)
        self.model.eval()
        images = self._load_batch(image_files)
        contexts = self.model.compute_contexts(images)
        try:
            period = vocabulary.words.index('.')
        except ValueError:
            period = -1
        return self._fused_beam.search(
            contexts, period, getattr(self.config, 'beam_size', 3))

    @torch.no_grad()
    def beam_search_device(self, image_files, vocabulary):
        """Device-resident beam search: per-step candidate scoring,
        top-k selection, '.'-termination and the bounded completed set
        all run on-GPU; the only host sync is the final result readout.

        Hypothesis semantics are the reference's (base_model.py:184-240):
        beam_size+1 expansion per live hypothesis, probability-PRODUCT
        scores (fp64, matching host float math), completed set bounded
        at beam_size, partial fallback when nothing completed."""
        config = self.config
        self.model.eval()
        W = beam_size = getattr(config, 'beam_size', 3)
        B = len(image_files)
        T = config.max_caption_length
        dev = self.device

        images = self._load_batch(image_files)
        contexts, init_memory, init_output = self.model.encode(images)
        H = init_memory.shape[1]

        try:
            period = vocabulary.words.index('.')
        except ValueError:
            period = -1

        # fixed W slots per image; dead slots carry score -inf
        NEG = float('-inf')
        scores = torch.full((B, W), NEG, dtype=torch.float64, device=dev)
        scores[:, 0] = 0.0  # log-space accumulator? no: product below
        scores = scores.exp()                     # [B,W]: 1, 0, 0
        seqs = torch.zeros(B, W, T, dtype=torch.int64, device=dev)
        lens = torch.zeros(B, W, dtype=torch.int64, device=dev)
        memory = init_memory.unsqueeze(1).repeat(1, W, 1).clone()
        output = init_output.unsqueeze(1).repeat(1, W, 1).clone()
        last_word = torch.zeros(B, W, dtype=torch.int64, device=dev)

        c_scores = torch.zeros(B, W, dtype=torch.float64, device=dev)
        c_seqs = torch.zeros(B, W, T, dtype=torch.int64, device=dev)
        c_lens = torch.zeros(B, W, dtype=torch.int64, device=dev)

        ctx_rep = contexts.repeat_interleave(W, dim=0)

        for t in range(T):
            mem2, out2, probs = self.model.decode_step(
                ctx_rep, last_word.reshape(-1),
                memory.reshape(B * W, H), output.reshape(B * W, H))
            top_p, top_w = probs.topk(beam_size + 1, dim=1)
            # candidate score = parent score * p(word)  [B, W*(K)]
            cand = (scores.unsqueeze(2)
                    * top_p.double().reshape(B, W, -1)).reshape(B, -1)
            cand_w = top_w.reshape(B, -1)
            K = beam_size + 1

            is_period = cand_w == period
            # ---- completed: merge period-candidates into the bounded
            # completed set (reference TopN(beam_size) push) ----
            comp_cand = torch.where(is_period, cand,
                                    torch.zeros_like(cand))
            merged_s = torch.cat([c_scores, comp_cand], dim=1)
            parent = torch.arange(W * K, device=dev).reshape(1, -1) \
                .expand(B, -1) // K
            new_seq = seqs.gather(
                1, parent.unsqueeze(2).expand(B, W * K, T)).clone()
            new_len = lens.gather(1, parent)
            step_seq = new_seq.scatter(
                2, new_len.clamp(max=T - 1).reshape(B, W * K, 1),
                cand_w.reshape(B, W * K, 1))
            step_len = (new_len + 1).clamp(max=T)
            merged_seq = torch.cat([c_seqs, step_seq], dim=1)
            merged_len = torch.cat([c_lens, step_len], dim=1)
            keep_s, keep_i = merged_s.topk(W, dim=1)
            c_scores = keep_s
            c_seqs = merged_seq.gather(
                1, keep_i.unsqueeze(2).expand(B, W, T))
            c_lens = merged_len.gather(1, keep_i)

            # ---- partial: best W non-period candidates ----
            part = torch.where(is_period,
                               torch.full_like(cand, NEG), cand)
            part = torch.nan_to_num(part, nan=NEG, neginf=NEG)
            sel_s, sel_i = part.topk(W, dim=1)
            scores = sel_s.clamp_min(0.0)
            sel_parent = sel_i // K
            seqs = step_seq.gather(
                1, sel_i.unsqueeze(2).expand(B, W, T))
            lens = step_len.gather(1, sel_i)
            last_word = cand_w.gather(1, sel_i)
            mem3 = mem2.reshape(B, W, H).gather(
                1, sel_parent.unsqueeze(2).expand(B, W, H))
            out3 = out2.reshape(B, W, H).gather(
                1, sel_parent.unsqueeze(2).expand(B, W, H))
            memory, output = mem3, out3

        # ---- readout (single host sync) ----
        c_scores_h = c_scores.cpu().numpy()
        c_seqs_h = c_seqs.cpu().numpy()
        c_lens_h = c_lens.cpu().numpy()
        p_scores_h = scores.cpu().numpy()
        p_seqs_h = seqs.cpu().numpy()
        p_lens_h = lens.cpu().numpy()

        results = []
        for k in range(B):
            use_partial = float(c_scores_h[k].max()) <= 0.0
            ss = p_scores_h[k] if use_partial else c_scores_h[k]
            qq = p_seqs_h[k] if use_partial else c_seqs_h[k]
            ll = p_lens_h[k] if use_partial else c_lens_h[k]
            order = ss.argsort()[::-1][:beam_size]
            caps = [CaptionData([int(v) for v in qq[i][:ll[i]]],
                                None, None, float(ss[i]))
                    for i in order if ss[i] > 0.0 or use_partial]
            if not caps:
                caps = [CaptionData([], None, None, 0.0)]
            results.append(caps)
        return results

    @torch.no_grad()
    def beam_search_host(self, image_files, vocabulary):
        """Host-heap beam search (the semantics reference; one topk
        sync per step)."""
        config = self.config
        self.model.eval()
        beam_size = getattr(config, 'beam_size', 3)
        B = len(image_files)

        images = self._load_batch(image_files)
        contexts, initial_memory, initial_output = self.model.encode(images)

        partial = []
        complete = []
        for k in range(B):
            init = CaptionData(sentence=[], memory=initial_memory[k],
                               output=initial_output[k], score=1.0)
            t = TopN(beam_size)
            t.push(init)
            partial.append(t)
            complete.append(TopN(beam_size))

        for idx in range(config.max_caption_length):
            # flatten all live hypotheses into one decode_step launch
            live = []          # (image_idx, CaptionData)
            for k in range(B):
                hyps = partial[k].extract()
                partial[k].reset()
                live.extend((k, h) for h in hyps)
            if not live:
                break

            img_idx = torch.tensor([k for k, _ in live],
                                   device=self.device)
            ctx = contexts.index_select(0, img_idx)
            last_word = torch.tensor(
                [h.sentence[-1] if h.sentence else 0 for _, h in live],
                dtype=torch.int64, device=self.device)
            last_memory = torch.stack([h.memory for _, h in live])
            last_output = torch.stack([h.output for _, h in live])

            memory, output, probs = self.model.decode_step(
                ctx, last_word, last_memory, last_output)

            # beam_size+1 most probable words per hypothesis
            top_p, top_w = probs.topk(beam_size + 1, dim=1)
            top_p = top_p.cpu().numpy()
            top_w = top_w.cpu().numpy()

            n_words = len(vocabulary.words)
            for row, (k, h) in enumerate(live):
                for w, s in zip(top_w[row], top_p[row]):
                    beam = CaptionData(h.sentence + [int(w)],
                                       memory[row], output[row],
                                       h.score * float(s))
                    if int(w) < n_words and vocabulary.words[int(w)] == '.':
                        complete[k].push(beam)
                    else:
                        partial[k].push(beam)

        results = []
        for k in range(B):
            if complete[k].size() == 0:
                complete[k] = partial[k]
            results.append(complete[k].extract(sort=True))
        return results

    # ------------------------------------------------------------------
    # checkpointing
    # ------------------------------------------------------------------

    def save(self):
        return ckpt.save(self.model, self.optimizer, self.config,
                         self.global_step)

    def load(self, model_file=None):
        self.global_step = ckpt.load(self.model, self.optimizer,
                                     self.config, model_file)
        if self.optimizer is not None:
            self.optimizer.step_count = max(self.optimizer.step_count,
                                            self.global_step)
        return self.global_step

    def load_cnn(self, data_path):
        return ckpt.load_cnn(self.model, data_path)
