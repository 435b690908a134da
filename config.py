"""Configuration for the MI355X-native Show-Attend-and-Tell framework.

Knob-name parity with the reference (`/root/reference/config.py:4-85`): every
hyperparameter the reference exposes exists here under the same name, so a user
of the reference can carry their edits over unchanged.  MI355X-specific knobs
(compute dtype, kernel backend, DP bucket sizing, hipGraph capture) are added at
the end — they have sane defaults and never need touching for parity runs.
"""


class Config(object):
    """Wrapper class for various (hyper)parameters."""

    def __init__(self):
        # about the model architecture (reference config.py:8-17)
        self.cnn = 'vgg16'               # 'vgg16' or 'resnet50'
        self.max_caption_length = 20
        self.dim_embedding = 512
        self.num_lstm_units = 512
        self.num_initalize_layers = 2    # 1 or 2 (reference spelling kept)
        self.dim_initalize_layer = 512
        self.num_attend_layers = 2       # 1 or 2
        self.dim_attend_layer = 512
        self.num_decode_layers = 2       # 1 or 2
        self.dim_decode_layer = 1024

        # about the weight initialization and regularization (config.py:20-27)
        self.fc_kernel_initializer_scale = 0.08
        self.fc_kernel_regularizer_scale = 1e-4
        self.fc_activity_regularizer_scale = 0.0
        self.conv_kernel_regularizer_scale = 1e-4
        self.conv_activity_regularizer_scale = 0.0
        self.fc_drop_rate = 0.5
        self.lstm_drop_rate = 0.3
        self.attention_loss_factor = 0.01

        # about the optimization (config.py:30-43)
        self.num_epochs = 30
        self.batch_size = 20
        self.optimizer = 'Adam'          # 'Adam', 'RMSProp', 'Momentum' or 'SGD'
        self.initial_learning_rate = 0.0001
        self.learning_rate_decay_factor = 1.0
        self.num_steps_per_decay = 100000
        self.clip_gradients = 5.0
        self.momentum = 0.0
        self.use_nesterov = True
        self.decay = 0.9
        self.centered = True
        self.beta1 = 0.9
        self.beta2 = 0.999
        self.epsilon = 1e-6

        # Clusterone environment paths (config.py:46-50) — kept for knob
        # parity; the MI355X launch path (torchrun/RCCL) does not use them
        self.path_to_local_logs = './summary'
        self.root_path_to_local_data = './data'
        self.local_repo = 'show-attend-and-tell'
        self.cloud_user_repo = 'Cheng-Lin-Li/show-attend-and-tell'
        self.cloud_path_to_data = 'data'

        # about the saver (config.py:53-55)
        self.save_period = 50
        self.save_dir = './data/models/'
        self.summary_dir = './summary/'

        # size-of-dataset caps — the reference's de-facto smoke-test knobs
        # (config.py:60-63)
        self.max_train_ann_num = 1000
        self.max_eval_ann_num = 20

        # about the vocabulary (config.py:66-67)
        self.vocabulary_file = './data/vocabulary.csv'
        self.vocabulary_size = 5000

        # about the training (config.py:70-74)
        self.train_image_dir = './data/train/images/'
        self.train_caption_file = './data/train/captions_train2014.json'
        self.temp_annotation_file = './data/train/anns.csv'
        self.temp_data_file = './data/train/data.npy'

        # about the evaluation (config.py:77-81)
        self.eval_image_dir = './data/val/images/'
        self.eval_caption_file = './data/val/captions_val2014.json'
        self.eval_result_dir = './data/val/results/'
        self.eval_result_file = './data/val/results.json'
        self.save_eval_result_as_image = True  # reference config.py:81

        # about the testing (config.py:83-85)
        self.test_image_dir = './data/test/images/'
        self.test_result_dir = './data/test/results/'
        self.test_result_file = './data/test/results.csv'

        # ------------------------------------------------------------------
        # MI355X-native knobs (new — no reference analog)
        # ------------------------------------------------------------------
        self.device = 'auto'             # 'auto' | 'cuda' | 'cpu'
        self.compute_dtype = 'bf16'      # 'bf16' | 'fp32' — CNN/decoder compute
        self.use_hip_kernels = True      # hand-written CDNA4 kernels on GPU
        self.use_hip_graph = True        # capture the train step in a hipGraph
        self.use_bptt = True             # fused hand-written BPTT over the
        #                                  T-step decoder (GPU bf16, default
        #                                  architecture only; False = per-op
        #                                  autograd loop, same numerics)
        self.allreduce_bucket_mb = 16    # DP gradient bucket size (xGMI-tuned)
        self.use_device_beam = True      # device-resident beam search (one
        #                                  host sync per batch; False = the
        #                                  host-heap reference path)
        self.use_fused_beam = False      # beam search through the fused,
        #                                  graph-captured inference engine
        #                                  (sat_amd/beam.py; GPU bf16, default
        #                                  architecture, beam <= 8; anything
        #                                  else keeps the paths above)
        self.use_glds_conv = True        # LDS-staged (glds) implicit-GEMM conv
        #                                  kernels for Cin<=128/Cout>=128 3x3
        #                                  layers (beats MIOpen per
        #                                  profiles/r01_conv_shapes.txt)
        self.synthetic_data = False      # synthetic COCO-shaped data (no files)
        self.synthetic_num_images = 640
        self.seed = 1234
        self.use_fused_optimizer = True  # RMSProp / Momentum / SGD through
        #                                  the chunk-table HIP kernels (graph-
        #                                  capturable; False = eager PyTorch
        #                                  math with host syncs).  Adam is
        #                                  always fused on the GPU.
        self.use_adam_chunk_norm = True  # Adam's norm and update over the
        #                                  chunk table (one partial per block,
        #                                  fixed-order sum: reproducible);
        #                                  False = the per-element-search
        #                                  pair with an atomic norm
        self.cache_frozen_conv_cast = True  # a frozen conv keeps its bf16
        #                                  weight and bias across forwards
        #                                  instead of casting them every step

        # input pipeline (sat_amd/data/pipeline.py); the defaults keep the
        # synchronous load-then-step loop
        self.num_loader_threads = 0      # > 0: that many threads (at most
        #                                  16) decode the coming batches'
        #                                  files while the GPU works
        self.prefetch_batches = 2        # how many batches they run ahead
        self.device_image_prep = False   # resize, mean and cast on the
        #                                  device from the decoded uint8
        #                                  images (same bits as the host
        #                                  path; real files, per-channel
        #                                  mean only)

        # Optional JSON overrides from the environment (testing / ops
        # hook): SAT_CONFIG_OVERRIDES='{"batch_size": 2, ...}'
        import json as _json
        import os as _os
        overrides = _os.environ.get('SAT_CONFIG_OVERRIDES')
        if overrides:
            for k, v in _json.loads(overrides).items():
                setattr(self, k, v)
