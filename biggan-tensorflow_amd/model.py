"""``BigGAN`` with the reference's ``generator`` / ``discriminator`` topology and train ops
(``/root/reference/BigGAN.py:246-715, 768-961``; option plumbing ``GANBase.py:13-55``) executing
eagerly on one MI355X per process.  One training iteration = D step then G step
(BigGAN.py:1061-1084); each step is one "run" with its own z, DiffAugment draws and one spectral-norm
power iteration per weight.

Out-of-scope reference features (alternative heads, the z-reconstruction head, d_final_conv)
are accepted as flags and rejected here with NotImplementedError.
"""
import copy
import os
import math
import time

import torch

from . import ops
from . import functional as Fn
from . import scope as S
from . import hip
from .ops import (fully_connected, resblock_up_condition, resblock_down, resblock, self_attention_2, conv, bn,
                  resblock_up_cond_deep, resblock_down_deep, upconv, g_conv, cond_bn, mixed_resblock,
                  prelu, relu, lrelu, tanh, alpha_helper_tanh, alpha_mask, global_sum_pooling, discriminator_loss,
                  generator_loss, glu, up_sample)
from .DiffAugment import DiffAugment, draw as draw_augment
from .utils import (orthogonal_regularizer, orthogonal_regularizer_fc, l2_regularizer, round_up, cls_loss_fn,
                    parse_cls_loss_type)


def _meta_2d(B, width):
    return torch.empty(B, width, device="meta")


class GANBase(object):
    """GANBase.py:13-55 (attribute plumbing, bn/conv option dicts, da_policy expansion)."""

    def __init__(self, args):
        self.dataset_name = args.dataset
        self.checkpoint_dir = args.checkpoint_dir
        self.sample_dir = args.sample_dir
        self.result_dir = args.result_dir
        self.log_dir = args.log_dir
        self.epoch = args.epoch
        self.iterations_per_epoch = args.iteration
        self.batch_size = args.batch_size
        self.virtual_batches = args.virtual_batches
        self.print_freq = args.print_freq
        self.save_freq = args.save_freq
        self.histogram_freq = int(getattr(args, "histogram_freq", 0) or 0)
        self.log_events = False               # train() writes the event file of trainlog.py only when this is set
        self.img_size = args.img_size
        self.bn_options = {"type": args.bn_type, "momentum": args.bn_momentum}       # GANBase.py:39-47
        if self.bn_options["type"] == 'batch_renorm':
            self.bn_options["renorm_clipping"] = {"rmax": args.bn_renorm_rmax, "dmax": args.bn_renorm_dmax}
            self.bn_options["renorm_momentum"] = args.bn_renorm_momentum
            self.bn_options["shared_renorm"] = args.bn_renorm_shared
        self.conv_options = {"padding_type": args.conv_padding, "sn": args.sn}       # GANBase.py:49-51
        self.da_policy = args.da_policy
        if self.da_policy == 'full':
            self.da_policy = 'color,translation,cutout'                               # GANBase.py:53-55


class BigGAN(GANBase):
    def __init__(self, args, device="cuda", store=None, process_group=None, seed=42):
        GANBase.__init__(self, args)
        self.model_name = "BigGAN"
        self.args = args
        self.device = torch.device(device)
        self.depth = args.img_size.bit_length() - 2                                   # BigGAN.py:19

        unsupported = [
            # (the reference accepts it and only re-splits z: no labels, no embedding; rejected as a likely mistake)
            ("cls_embedding without n_labels", args.cls_embedding and args.n_labels <= 0),
            ("g_final_layer", args.g_final_layer), ("multi_head", args.multi_head),
            ("z_reconstruct", args.z_reconstruct), ("d_final_conv", args.d_final_conv),
        ]
        bad = [n for n, v in unsupported if v]
        if bad:
            raise NotImplementedError("flags outside the MI355X hot path (SURVEY.md section 8): " + ", ".join(bad))
        if args.c_dim not in (1, 3, 4):                                                # TF decode_png: 1, 3 or 4 channels
            raise ValueError("--c_dim %d: images have 1 (grayscale), 3 (RGB) or 4 (RGBA) channels" % args.c_dim)
        self.gan_type = args.gan_type
        self.d_loss_func = args.d_loss_func if args.d_loss_func else self.gan_type     # BigGAN.py:127-128
        if self.gan_type not in Fn.GAN_LOSS_KINDS or self.d_loss_func not in Fn.GAN_LOSS_KINDS:
            raise ValueError("--gan_type / --d_loss_func %s / %s: available: %s"
                             % (self.gan_type, self.d_loss_func, ", ".join(sorted(Fn.GAN_LOSS_KINDS))))
        self.relativistic = self.gan_type.startswith('ra-')
        if 'wgan' in self.d_loss_func:                                                 # BigGAN.py:130-138
            self.gradient_penalty_type = self.gan_type
        elif 'dragan' in self.d_loss_func:
            self.gradient_penalty_type = 'dragan'
        else:
            self.gradient_penalty_type = None
        self.use_gradient_penalty = bool(self.gradient_penalty_type)
        if self.use_gradient_penalty and self.gradient_penalty_type not in ('wgan-gp', 'wgan-lp', 'dragan'):
            raise ValueError("gradient penalty type %r (BigGAN.py:736-740 knows wgan-gp, wgan-lp, dragan)"
                             % self.gradient_penalty_type)
        self.ld = args.ld

        self.activation = args.activation                                              # BigGAN.py:71-83
        if self.activation == 'relu':
            self.activation_fn = relu
        elif self.activation == 'prelu':
            self.activation_fn = prelu
        elif self.activation == 'lrelu':
            def lrelu_p(alpha):
                def lrelu_a(x):
                    return lrelu(x, alpha)
                return lrelu_a
            self.activation_fn = lrelu_p(0.2)                                          # BigGAN.py:76-81
        else:
            raise ValueError("Unknown activation function: " + str(self.activation))

        self.ch = args.ch
        self.d_ch = args.d_ch if args.d_ch > 0 else args.ch                            # BigGAN.py:153-154
        self.upsampling_method = args.upsampling_method
        self.downsampling_method = args.downsampling_method
        self.g_conv = args.g_conv
        self.g_grow_factor = args.g_grow_factor
        self.d_grow_factor = args.d_grow_factor
        self.g_regularization_method = args.g_regularization
        self.g_regularization_factor = args.g_regularization_factor
        self.g_sa_size = args.g_sa_size if args.g_sa_size != 0 else args.sa_size       # BigGAN.py:110-117
        self.d_sa_size = args.d_sa_size if args.d_sa_size != 0 else args.sa_size
        self.z_dim = args.z_dim
        self.first_split_ratio = args.first_split_ratio
        if self.z_dim % self.depth != 0 and self.first_split_ratio == 1:               # BigGAN.py:122-124
            self.z_dim = self.z_dim + self.depth - self.z_dim % self.depth
        self.g_flood, self.d_flood = args.g_flood, args.d_flood
        self.n_critic = args.n_critic
        self.sn = args.sn
        self.d_use_bias = args.bias_in_d
        self.bias_in_sa = args.bias_in_sa
        self.bn_in_d = args.bn_in_d
        self.c_dim = args.c_dim
        self.alpha_mask = self.c_dim == 4 and args.alpha_mask                          # BigGAN.py:616
        self.g_alpha_helper = self.c_dim == 4 and args.g_alpha_helper                  # BigGAN.py:572
        self.g_rgb_mix_kernel = args.g_rgb_mix_kernel
        self.z_trunc_train = args.z_trunc_train
        self.g_learning_rate, self.d_learning_rate = args.g_lr, args.d_lr
        self.beta1, self.beta2 = args.beta1, args.beta2
        self.moving_decay = args.moving_decay
        self.d_compat_use_sn_in_critic_output = args.d_compat_use_sn_in_critic_output
        self.extension_32 = getattr(args, "extension_32", False)
        # the discriminator's reconstruction heads (BigGAN.py:42-53); halfres implies the coarse head
        self.d_reconstruction_halfres = bool(args.d_reconstruction_halfres)
        self.d_reconstruction = bool(args.d_reconstruction or args.d_reconstruction_halfres)
        self.d_reconstruction_texture = bool(args.d_reconstruction_texture)
        self.d_recon_ch, self.d_recon_ld = args.d_recon_ch, args.d_recon_ld
        self.d_tex_recon_ch, self.d_tex_recon_ld = args.d_tex_recon_ch, args.d_tex_recon_ld
        self.d_tex_recon_feat_size = args.d_tex_recon_feat_size
        self.d_tex_recon_patch_div = args.d_tex_recon_patch_div
        self.d_recon_bn_after_act = bool(args.d_recon_bn_after_act)
        self.d_save_recon_samples = bool(args.d_save_recon_samples)
        # in-training sample grids (BigGAN.py:168-183)
        self.sample_num = args.sample_num
        self.static_sample_z = bool(args.static_sample_z)
        self.static_sample_seed = args.static_sample_seed
        self.z_trunc_sample = bool(args.z_trunc_sample)
        self.save_morphs = bool(args.save_morphs)
        self.save_cls_samples = bool(args.save_cls_samples)
        self.sample_ema = args.sample_ema
        if self.sample_ema not in ('ema', 'noema', 'both'):
            raise ValueError('Invalid mode for sample_ema specified')
        self.generate_noema_samples = self.sample_ema != 'ema'
        self.generate_ema_samples = self.sample_ema != 'noema'
        if self.save_morphs and int(math.floor(math.sqrt(self.sample_num))) < 2:
            raise ValueError("--save_morphs needs --sample_num >= 4 (the blend weights divide by the grid side - 1)")
        # fresh sample latents (--static_sample_z false) have a generator of their own: looking at samples never
        # advances the draws of the training run (self.gen)
        self.sample_gen = torch.Generator(device="cpu")
        self.sample_gen.manual_seed((int(self.static_sample_seed) + 1) % (1 << 63))
        self.labels = None                     # the dataset's label table (open_dataset); None: synthetic one-hots
        self.label_table = None                # the same table as a device fp32 [rows, n_labels] (draw_labels)
        self._static_set = None                # (z, class vectors) of the static sample set, drawn on first use
        # in-training quality score (extension flags --swd_freq / --swd_images; metrics.py)
        self.swd_freq = int(getattr(args, "swd_freq", 0) or 0)
        self.swd_images = int(getattr(args, "swd_images", 2048) or 2048)
        self._monitors = {}                    # kind -> its metrics.Monitor with the kept real set and the draws of the run,
                                               # built at the kind's first event ("swd", "msssim", "ps", "prdc")
        # nearest training images (extension flags --nn_freq / --nn_k / --nn_size / --nn_images; neighbours.py)
        self.nn_freq = int(getattr(args, "nn_freq", 0) or 0)
        self.nn_k = int(getattr(args, "nn_k", 3) or 3)
        self.nn_size = int(getattr(args, "nn_size", 64) or 64)
        self.nn_images = int(getattr(args, "nn_images", 0) or 0)
        self._nn = None                        # neighbours.NearestSet with the resident training set, built at the first event
        # in-training diversity score (extension flags --msssim_freq / --msssim_pairs; metrics.py)
        self.msssim_freq = int(getattr(args, "msssim_freq", 0) or 0)
        self.msssim_pairs = int(getattr(args, "msssim_pairs", 1024) or 1024)
        # in-training frequency check (extension flags --ps_freq / --ps_images; metrics.py)
        self.ps_freq = int(getattr(args, "ps_freq", 0) or 0)
        self.ps_images = int(getattr(args, "ps_images", 1024) or 1024)
        # in-training precision / recall / density / coverage (extension flags --pr_freq / --pr_images / --pr_k /
        # --pr_size; metrics.py)
        self.pr_freq = int(getattr(args, "pr_freq", 0) or 0)
        self.pr_images = int(getattr(args, "pr_images", 4096))
        self.pr_k = int(getattr(args, "pr_k", 3))
        self.pr_size = int(getattr(args, "pr_size", 64))
        # singular-value monitor (extension flags --sv_freq / --sv_k / --sv_iters / --sv_tol; spectrum.py)
        self.sv_freq = int(getattr(args, "sv_freq", 0) or 0)
        self.sv_k = int(getattr(args, "sv_k", 3))
        self.sv_iters = int(getattr(args, "sv_iters", 8))
        self.sv_tol = float(getattr(args, "sv_tol", 1e-2))
        if not 1 <= self.sv_k <= 4:
            raise ValueError("--sv_k %d: 1..4 singular values per weight" % self.sv_k)
        if not 1 <= self.sv_iters <= 256:
            raise ValueError("--sv_iters %d: 1..256 iterations per round" % self.sv_iters)
        if not self.sv_tol > 0.0:
            raise ValueError("--sv_tol %s: a positive residual" % self.sv_tol)
        self._sv = None                        # spectrum.SingularValues with the basis of the run, built at the first event
        self.recon_plan = self._recon_plan()
        self.deep = args.deep                                                          # BigGAN.py:20
        self.g_mixed_resblocks = args.g_mixed_resblocks                                # BigGAN.py:40-41
        self.g_mixed_resblock_ch_div = args.g_mixed_resblock_ch_div
        self.cls_embedding = args.cls_embedding                                        # BigGAN.py:24-28
        self.cls_embedding_size = args.cls_embedding_size
        if self.cls_embedding and self.cls_embedding_size == 0:
            self.cls_embedding_size = self.round_up(math.pow(args.n_labels, 0.88) + 24, 8)
        self.cls_embedding_concat = args.cls_embedding_concat
        self.shared_z_dim = args.shared_z
        self.g_z_dense_concat = args.g_z_dense_concat
        # (BigGAN.py:278: mixed_conv_z_idx also selects it, but needs --g_final_layer, which stays rejected above)
        self.new_z_dist = bool(self.cls_embedding or self.shared_z_dim > 0 or self.g_z_dense_concat)
        self.n_labels = args.n_labels                                                  # BigGAN.py:22-23
        self.acgan = self.n_labels > 0
        self.virtual_batches = max(int(args.virtual_batches), 1)
        if self.acgan:                                                                 # BigGAN.py:91-100
            self.cls_loss_type = args.cls_loss_type
            parse_cls_loss_type(self.cls_loss_type, self.n_labels)     # utils.py:339-375: a bad spec fails here
            self.d_cls_loss_weight = args.d_cls_loss_weight
            self.g_cls_loss_weight = args.g_cls_loss_weight
            self.d_compat_use_sn_in_classification = args.d_compat_use_sn_in_classification
            if args.cls_loss_weights != '':
                self.cls_loss_weights = list(map(float, open(args.cls_loss_weights).read().split()))
                if len(self.cls_loss_weights) != self.n_labels:
                    raise ValueError('Number of class loss weights does not match n_labels (' +
                                     str(len(self.cls_loss_weights)) + " vs. " + str(self.n_labels) + ")")
            else:
                self.cls_loss_weights = [1.0] * self.n_labels

        # arithmetic / storage policy (extension flag --precision): must be set before build_model() sizes the
        # packed-weight buffers of the spectral-norm batches
        self.precision = getattr(args, "precision", None) or "fp32"
        Fn.set_precision(self.precision)
        self.store = store if store is not None else S.VariableStore(self.device, seed)
        S.set_default_store(self.store)
        self.pg = process_group
        self.world = 1
        self.rank = 0
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        self.gen = torch.Generator(device=self.device) if self.device.type == "cuda" else None
        if self.gen is not None:
            self.gen.manual_seed(1234 + self.rank)
        self.built = False

    ##################################################################################
    # Generator  (BigGAN.py:236-582)
    ##################################################################################
    def round_up(self, val, multiple):
        return (int(val) + multiple - 1) // multiple * multiple

    def scale_channels(self, ch, factor):
        return self.round_up(int(ch * factor), 8)

    def g_channels_for_block(self, b_i, b_count):
        return self.scale_channels(self.ch, self.g_grow_factor ** (b_count - b_i - 1))

    def g_block_info(self):                                                            # BigGAN.py:290-294
        s = self.img_size
        if s == 64: info = {"counts": [1, 1, 1, 1], "sa_index": 3}
        elif s == 128: info = {"counts": [1, 1, 1, 1, 1], "sa_index": 4}
        elif s == 256: info = {"counts": [1, 2, 1, 1, 1], "sa_index": 3}
        elif s == 512: info = {"counts": [1, 2, 1, 1, 2], "sa_index": 3}
        elif s == 32 and self.extension_32: info = {"counts": [1, 1, 1], "sa_index": 2}
        else: raise ValueError("Invalid image size specified: " + str(self.img_size))
        if self.g_sa_size != 0:
            self.set_sa_index(info, self.g_sa_size)
        return info

    def d_block_info(self):                                                            # BigGAN.py:607-611
        s = self.img_size
        if s == 64: info = {"counts": [1, 1, 1, 1], "sa_index": 1}
        elif s == 128: info = {"counts": [1, 1, 1, 1, 1], "sa_index": 1}
        elif s == 256: info = {"counts": [1, 1, 1, 2, 1], "sa_index": 2}
        elif s == 512: info = {"counts": [1, 2, 1, 1, 2], "sa_index": 2}
        elif s == 32 and self.extension_32: info = {"counts": [1, 1, 1], "sa_index": 1}
        else: raise ValueError("Invalid image size specified: " + str(self.img_size))
        if self.d_sa_size != 0:
            self.set_sa_index(info, self.d_sa_size, scaling_down=True)
        return info

    def set_sa_index(self, block_info, sa_size, scaling_down=False):
        """BigGAN.py:1457-1480."""
        if sa_size < 0:
            block_info["sa_index"] = -1
            return
        cur_f_size = self.img_size if scaling_down else 4
        for i, bs in enumerate(block_info["counts"]):
            for j in range(bs):
                if scaling_down:
                    cur_f_size //= 2
                else:
                    cur_f_size *= 2
            if scaling_down:
                met_goal = cur_f_size <= sa_size
            else:
                met_goal = cur_f_size >= sa_size
            if met_goal or i == len(block_info["counts"]) - 1:
                block_info["sa_index"] = i + 1
                break
        if cur_f_size != sa_size:
            print("Warning: moving self-attention to " + str(cur_f_size) + "x" + str(cur_f_size) + " feature maps")

    def z_split_sizes(self):                                                           # BigGAN.py:280-288
        if self.first_split_ratio > 1:
            split_dim = self.z_dim // (self.depth - 1 + self.first_split_ratio)
            first_split_dim = self.z_dim - (self.depth - 1) * split_dim
        else:
            split_dim = self.z_dim // self.depth
            first_split_dim = split_dim
        return [first_split_dim] + ([split_dim] * (self.depth - 1))

    def generator(self, z, cls_z=None, is_training=True, reuse=False, custom_getter=None, simple_head=False):
        opt = {"sn": self.sn, "is_training": is_training, "upsampling_method": self.upsampling_method,
               "g_conv": self.g_conv, "act": self.activation_fn, "self_attention_bias": self.bias_in_sa,
               "bn": copy.deepcopy(self.bn_options), "conv": copy.deepcopy(self.conv_options)}
        if is_training:                                                                # BigGAN.py:257-274
            m = self.g_regularization_method
            if m == 'none':
                opt["conv"]["regularizer"] = None
                opt["fc_regularizer"] = None
            elif m in ('ortho', 'ortho_cosine'):
                opt["conv"]["regularizer"] = orthogonal_regularizer(self.g_regularization_factor, type=m)
                opt["fc_regularizer"] = orthogonal_regularizer_fc(self.g_regularization_factor, type=m)
            elif m == 'l2':
                opt["conv"]["regularizer"] = l2_regularizer(self.g_regularization_factor)
                opt["fc_regularizer"] = l2_regularizer(self.g_regularization_factor)
            else:
                raise ValueError("Unknown regularization method: " + str(m))
        else:
            opt["conv"]["regularizer"] = None
            opt["fc_regularizer"] = None

        self._sn_prefetch("generator", z)
        if self.new_z_dist:
            with S.variable_scope("generator", reuse=reuse):
                block_info = self.g_block_info()
                levels = self._latent_levels(z, cls_z, opt, block_info)
                return self._generator_trunk(levels, opt, block_info, new_z_dist=True)
        with S.variable_scope("generator", reuse=reuse):
            block_info = self.g_block_info()
            split_sizes = self.z_split_sizes()
            z2 = z.reshape(z.shape[0], -1)
            z_split = list(torch.split(z2, split_sizes, dim=-1))                       # BigGAN.py:335 (views)
            clsz_size = 0
            if self.acgan:                                                             # BigGAN.py:346-365
                clsz_size = self.n_labels
                if z.device.type == "meta":
                    z_split = [torch.empty(zz.shape[0], zz.shape[1] + clsz_size, device="meta") for zz in z_split]
                else:
                    cz = cls_z.reshape(-1, clsz_size)
                    z_split = [torch.cat([zz, cz], dim=-1) for zz in z_split]
                split_sizes = [sz + clsz_size for sz in split_sizes]
            next_zi = [0]

            def next_z_split():
                zi = next_zi[0]
                next_zi[0] += 1
                return z_split[zi], split_sizes[zi]

            return self._generator_trunk([next_z_split() for _ in range(len(z_split))], opt, block_info)

    def new_z_split_sizes(self, block_info):                                           # BigGAN.py:314-333
        """z split by weights: [0 (shared slot)] + [first_split_ratio] + [1 per block]; the remainder goes to the first
        level, the shared slot gets --shared_z.  -> (sizes, shared slot or None, first slot, block slots)."""
        weights = []
        shared_idx = None
        if self.shared_z_dim > 0:
            shared_idx = len(weights)
            weights.append(0.0)
        first_idx = len(weights)
        weights.append(self.first_split_ratio)
        block_idx = []
        for count in block_info["counts"]:
            for _ in range(count):
                block_idx.append(len(weights))
                weights.append(1.0)
        total = sum(weights)
        nonshared = self.z_dim - self.shared_z_dim
        sizes = [int(w / total * nonshared) for w in weights]
        sizes[first_idx] += nonshared - sum(sizes)
        if shared_idx is not None:
            sizes[shared_idx] = self.shared_z_dim
        return sizes, shared_idx, first_idx, block_idx

    def _latent_levels(self, z, cls_z, opt, block_info):
        """BigGAN.py:335-424 (new_z_dist): class embedding, shared z and the per-level dense layers.  Every level's vector
        is kept as a list of column pieces (source, first column, width) of a few source tensors (z, the labels, the
        embedding, the shared projection, the level's own dense layer) and materialised by ONE fan-out launch per stage
        (functional.LatentFanoutFn) as column views of one packed buffer; backward reduces each source's gradient over
        all levels in one launch.  -> [(vector, width)] of the first level, then of every block."""
        opt["cbn_group_dz"] = True                # (ops._cbn_prefetch: the block projections' latent needs a gradient)
        meta = z.device.type == "meta"
        B = z.shape[0]
        sizes, shared_idx, first_idx, block_idx = self.new_z_split_sizes(block_info)
        srcs = [z.reshape(B, -1)]
        pieces, off = [], 0
        for sz in sizes:
            pieces.append([(0, off, sz)] if sz > 0 else [])
            off += sz
        zvec = list(sizes)

        def add_src(t):
            srcs.append(t)
            return len(srcs) - 1

        def materialise(slots):
            """Per slot: one tensor.  Single-piece slots of an existing source are column views of it (no launch)."""
            if meta:
                return [_meta_2d(B, sum(p[2] for p in pieces[i])) for i in slots]
            if all(len(pieces[i]) == 1 for i in slots):
                return [srcs[pieces[i][0][0]][:, pieces[i][0][1]:pieces[i][0][1] + pieces[i][0][2]] for i in slots]
            used = sorted({p[0] for i in slots for p in pieces[i]})
            segs, widths = [], []
            for oi, i in enumerate(slots):
                col = 0
                for si, sc, w in pieces[i]:
                    segs.append((used.index(si), sc, oi, col, w))
                    col += w
                widths.append(col)
            return list(Fn.LatentFanoutFn.apply(widths, segs, *[srcs[u] for u in used]))

        cls_pieces = []
        if self.acgan:                                                                 # BigGAN.py:346-365
            lab = add_src(_meta_2d(B, self.n_labels) if meta else cls_z.reshape(B, self.n_labels))
            cls_pieces = [(lab, 0, self.n_labels)]
            if self.cls_embedding:
                with S.variable_scope('cls_embed'):
                    e = fully_connected(srcs[lab], units=self.cls_embedding_size, scope='dense1', opt=opt)
                    e = add_src(opt["act"](e))
                emb = [(e, 0, self.cls_embedding_size)]
                cls_pieces = cls_pieces + emb if self.cls_embedding_concat else emb
            for i in range(len(pieces)):
                if self.g_z_dense_concat and i == shared_idx:
                    continue
                pieces[i] = pieces[i] + cls_pieces
                zvec[i] += sum(p[2] for p in cls_pieces)

        if shared_idx is not None:                                                     # BigGAN.py:367-392
            zd = sizes[shared_idx]
            with S.variable_scope('shared_z'):
                if self.g_z_dense_concat:
                    f_width = self.round_up(zd * 0.5, 8)
                    f_in = pieces[shared_idx] + cls_pieces
                else:
                    f_width = self.round_up(zd * 1.5, 8)
                    f_in = pieces[shared_idx]
                pieces.append(f_in)                                                    # (a scratch slot for the input)
                x_in = materialise([len(pieces) - 1])[0]
                pieces.pop()
                d = fully_connected(x_in, units=f_width, scope='dense1', opt=opt)
                d = add_src(opt["act"](d))
            if self.g_z_dense_concat:
                shared_pieces = pieces[shared_idx] + [(d, 0, f_width)]
                zvec[shared_idx] += f_width
            else:
                shared_pieces = [(d, 0, f_width)]
                zvec[shared_idx] = f_width
            for i in range(len(pieces)):
                if i != shared_idx:
                    pieces[i] = pieces[i] + shared_pieces
                    zvec[i] += zvec[shared_idx]

        level_idx = [first_idx] + block_idx
        dense_idx = ([first_idx] if self.args.g_first_level_dense_layer else []) + \
                    (block_idx if self.args.g_other_level_dense_layer else [])
        final = dict(zip(level_idx, materialise(level_idx)))
        if dense_idx:                                                                  # BigGAN.py:394-424
            concat_slots = []
            for zi in dense_idx:
                with S.variable_scope('z' + str(zi)):
                    factor = 1.5 if zi == first_idx else 1.0
                    if self.g_z_dense_concat:
                        factor = (factor - 1.0) * 2.0 + 1.0
                        f_width = self.round_up((zvec[zi] * 0.33) * factor, 8)
                    else:
                        f_width = self.round_up((sizes[zi] * 0.75 + zvec[zi] * 0.5) * factor, 8)
                    layer_z = fully_connected(final[zi], units=f_width, scope='dense1', opt=opt)
                    layer_z = opt["act"](layer_z)
                if self.g_z_dense_concat:
                    pieces[zi] = pieces[zi] + [(add_src(layer_z), 0, f_width)]
                    zvec[zi] += f_width
                    concat_slots.append(zi)
                else:
                    final[zi] = layer_z
                    zvec[zi] = f_width
            if concat_slots:        # one more stage: [level | dense(level)], gathered from the sources again
                final.update(zip(concat_slots, materialise(concat_slots)))
        return [(final[i], zvec[i]) for i in level_idx]

    def _generator_trunk(self, levels, opt, block_info, new_z_dist=False):
        """BigGAN.py:427-580: the first dense layer, the up blocks and the head.  ``levels``: (vector, width) of the first
        level, then of every block.  With ``new_z_dist`` the per-level dense layers have run already (_latent_levels)."""
        levels = iter(levels)

        def next_z_split():
            return next(levels)

        counts = block_info["counts"]
        ch_mul = 2 ** (len(counts) - 1)                                            # BigGAN.py:427
        ch = self.g_channels_for_block(0, len(counts))

        layer_z, z_dim = next_z_split()
        f_width = self.round_up(z_dim * 1.85, 8)                                   # BigGAN.py:433 (z_dim includes the labels)
        if new_z_dist:                                                             # BigGAN.py:444
            x = fully_connected(layer_z, units=4 * 4 * ch, scope='first/dense', opt=opt)
        elif not self.args.g_first_level_dense_layer:                              # BigGAN.py:444
            x = fully_connected(layer_z, units=4 * 4 * ch, scope='dense', opt=opt)
        elif self.activation_fn is relu:                                           # BigGAN.py:434-438
            x = fully_connected(layer_z, units=f_width, scope='dense1', opt=opt)
            x = relu(x)
            x = fully_connected(x, units=4 * 4 * ch, scope='dense2', opt=opt)
        else:
            with S.variable_scope('first'):                                        # BigGAN.py:440-443
                x = fully_connected(layer_z, units=f_width, scope='dense1', opt=opt)
                x = opt["act"](x)
                x = fully_connected(x, units=4 * 4 * ch, scope='dense2', opt=opt)
        x = ops._resident_out(x.reshape(-1, 4, 4, ch))                             # BigGAN.py:446 (bf16 trunk from here)

        b_i = 0
        for block_count in counts:                                                 # BigGAN.py:449-489
            x = self._grad_mark(x, 'resblock_up_' + str(ch_mul))
            scope = 'resblock_up_' + str(ch_mul)
            for sb_i in range(block_count):
                layer_z, z_dim = next_z_split()
                if block_count > 1:
                    scope = scope + '_' + str(sb_i)                                # cumulative (BigGAN.py:455)
                if self.args.g_other_level_dense_layer and not new_z_dist:         # BigGAN.py:457-462
                    with S.variable_scope('z' + str(ch_mul)):
                        zw = self.round_up(z_dim * 1.25, 8)                        # (z_dim includes the labels)
                        layer_z = fully_connected(layer_z, units=zw, scope='dense1', opt=opt)
                        layer_z = opt["act"](layer_z)
                is_last_block = sb_i == block_count - 1 and b_i == len(counts) - 1
                if self.args.g_no_last_resblock and is_last_block:                 # BigGAN.py:468-473
                    with S.variable_scope(scope):
                        x = upconv(x, ch, use_bias=False, opt=opt)
                        x = cond_bn(x, layer_z, opt=opt)
                        x = opt["act"](x)
                        x = g_conv(x, ch, use_bias=False, opt=opt)
                elif self.deep:                                                    # BigGAN.py:475-477
                    x = resblock_up_cond_deep(x, layer_z, channels_out=ch, use_bias=True, opt=opt, scope=scope)
                    x = resblock_up_cond_deep(x, layer_z, channels_out=ch, upscale=False, use_bias=True, opt=opt,
                                              scope=scope + "_2")
                else:
                    x = resblock_up_condition(x, layer_z, channels=ch, use_bias=False, opt=opt, scope=scope)
            b_i += 1
            if b_i == block_info["sa_index"]:
                x = self_attention_2(x, channels=ch, opt=opt, scope='self_attention')
            if self.g_mixed_resblocks:                                             # BigGAN.py:485-486
                x = mixed_resblock(x, self.round_up(ch / self.g_mixed_resblock_ch_div, 8), ch, opt=opt,
                                   scope='res_mixed' + str(ch_mul))
            ch = self.g_channels_for_block(b_i, len(counts))
            ch_mul = ch_mul // 2

        x = self._grad_mark(x, 'tail')
        x = ops._bn_act(x, None, opt)   # BigGAN.py:491-492
        x = conv(x, channels=self.c_dim, kernel=self.g_rgb_mix_kernel, stride=1, pad=1, use_bias=False, opt=opt,
                 scope='G_logit')                                                  # BigGAN.py:570
        if self.g_alpha_helper:                                                    # BigGAN.py:572-580
            return alpha_helper_tanh(x)
        x = tanh(x)                                                                # BigGAN.py:580
        return x

    ##################################################################################
    # Discriminator  (BigGAN.py:588-715)
    ##################################################################################
    def d_channels_for_block(self, b_i):
        return self.scale_channels(self.d_ch, self.d_grow_factor ** b_i)

    def make_opt_with_sn(self, src_opt, sn):
        """BigGAN.py:1482-1487."""
        sn_opt = copy.copy(src_opt)
        sn_opt["conv"] = copy.copy(src_opt["conv"])
        sn_opt["sn"] = sn
        sn_opt["conv"]["sn"] = sn
        return sn_opt

    def d_group_sizes(self):
        """Side of the feature map after each block group of the discriminator (where a reconstruction head may sit)."""
        sizes, s = [], self.img_size
        for count in self.d_block_info()["counts"]:
            s //= 2 ** count
            sizes.append(s)
        return sizes

    def _recon_plan(self):
        """Where the reconstruction heads attach and how deep they are (BigGAN.py:639-661), checked at construction.
        The layer count is log2(target / attach size): the reference's ``depth - 3`` reaches the target only after
        --g_final_layer has bumped ``depth`` (reconstruction heads, deviation 1)."""
        plan = {}
        if not (self.d_reconstruction or self.d_reconstruction_texture):
            return plan
        sizes = self.d_group_sizes()
        if self.d_reconstruction:
            if 8 not in sizes:
                raise ValueError("--d_reconstruction attaches to the 8x8 feature map, but at --img_size %d the block groups "
                                 "of the discriminator end at %s" % (self.img_size, ", ".join(map(str, sizes))))
            target = self.img_size // 2 if self.d_reconstruction_halfres else self.img_size
            plan["coarse"] = {"size": 8, "target": target, "layers": int(math.log2(target // 8))}
        if self.d_reconstruction_texture:
            fs, div = self.d_tex_recon_feat_size, self.d_tex_recon_patch_div
            if fs not in sizes:
                raise ValueError("--d_tex_recon_feat_size %d: at --img_size %d the block groups of the discriminator end "
                                 "at %s" % (fs, self.img_size, ", ".join(map(str, sizes))))
            if div < 1 or fs % div or self.img_size % div:
                raise ValueError("--d_tex_recon_patch_div %d must divide the feature size %d and the image size %d"
                                 % (div, fs, self.img_size))
            patch, feat_patch = self.img_size // div, fs // div
            plan["texture"] = {"size": fs, "patch": patch, "feat_patch": feat_patch, "f": self.img_size // fs,
                               "layers": int(math.log2(patch // feat_patch))}
        return plan

    def random_crop_offsets(self, img_shape, crop_size):
        """BigGAN.py:1489-1493: int32 offsets, uniform in [0, size - crop_size], one per sample (only element [0] is
        used, for the whole batch: BigGAN.py:656-657).  They stay on the device.  Under data parallelism rank 0's draw
        is used by every rank, so that the ranks crop one window as one GPU at the global batch would."""
        n = int(img_shape[0])
        out = []
        for side in (img_shape[1], img_shape[2]):
            out.append(torch.randint(0, int(side) - crop_size + 1, (n,), dtype=torch.int32, device=self.device,
                                     generator=self.gen))
        if self.world > 1:
            src = torch.distributed.get_global_rank(self.pg, 0) if self.pg is not None else 0
            for t in out:
                torch.distributed.broadcast(t, src=src, group=self.pg)
        return out[0], out[1]

    def simple_upscale(self, x, ch, scope, opt):
        """BigGAN.py:744-753: nearest 2x, conv to 2 ch, bn, glu (glu then bn with --d_recon_bn_after_act)."""
        with S.variable_scope(scope):
            x = up_sample(x)
            x = conv(x, channels=ch * 2, kernel=3, pad=1, stride=1, opt=opt)
            if not self.d_recon_bn_after_act:
                return ops.bn_glu(x, opt=opt)                      # bn, then glu: one apply kernel
            return bn(glu(x), opt=opt)

    def simple_upscaler(self, x, layers=3, scope="upscaler", base_width=64, opt={}, _pre_tanh=False):
        """BigGAN.py:755-762.  ``_pre_tanh`` (extension): return the image conv's output; the loss kernel applies the
        tanh itself (functional.ReconLossFn)."""
        with S.variable_scope(scope):
            for li in range(layers):
                x = self.simple_upscale(x, base_width * 2 ** (layers - li - 1), "upscale" + str(li), opt=opt)
            x = conv(x, channels=self.c_dim, kernel=3, pad=1, stride=1, opt=opt)
            return x if _pre_tanh else tanh(x)

    def _recon_heads(self, x, outputs, opt, recon):
        """The heads that attach to a feature map of x's size (BigGAN.py:639-661) -> x for the next block.  The map then
        has more than one consumer: it is forked, so that the branch gradients meet in one buffer."""
        size = x.shape[1]
        heads = [k for k in ("coarse", "texture") if k in self.recon_plan and self.recon_plan[k]["size"] == size]
        if not heads:
            return x
        branches = ops._fork(x, 1 + len(heads))
        for k, xb in zip(heads, branches[1:]):
            plan = self.recon_plan[k]
            if k == "coarse":
                outputs["coarse_logits"] = self.simple_upscaler(xb, base_width=self.d_recon_ch, layers=plan["layers"],
                                                                opt=opt, _pre_tanh=True)
            else:
                ro_x, ro_y = recon["offsets"]
                outputs["rnd_offset_x"], outputs["rnd_offset_y"] = ro_x, ro_y
                fp = plan["feat_patch"]
                if ops._is_meta(xb):
                    crop = torch.empty(xb.shape[0], fp, fp, xb.shape[3], device="meta")
                else:                           # (crop_to_bounding_box: the first offset is the height offset)
                    crop = Fn.CropAtFn.apply(xb, ro_x, ro_y, fp)
                outputs["texture_logits"] = self.simple_upscaler(crop, base_width=self.d_tex_recon_ch,
                                                                 layers=plan["layers"], opt=opt, scope="tex_upscaler",
                                                                 _pre_tanh=True)
        return branches[0]

    def discriminator(self, x, is_training=True, reuse=False, _recon=None):
        """``_recon`` (extension): set by the real call of the D step only - {"offsets": (ro_x, ro_y) or None}; the
        reconstruction heads run in that call and leave their pre-tanh images in the outputs."""
        opt = {"sn": self.sn, "is_training": is_training, "bn_in_d": self.bn_in_d, "act": self.activation_fn,
               "downsampling_method": self.downsampling_method, "self_attention_bias": self.bias_in_sa,
               "bn": copy.deepcopy(self.bn_options), "conv": copy.deepcopy(self.conv_options)}
        outputs = {}
        self._sn_prefetch("discriminator", x)
        if _recon is not None:
            self._sn_prefetch("d_recon", x)
        with S.variable_scope("discriminator", reuse=reuse):
            if self.alpha_mask:                                                        # BigGAN.py:616-619
                x = alpha_mask(x)
            ch = self.d_channels_for_block(0)
            block_info = self.d_block_info()
            b_i = 0
            ch_mul = 1
            for block_count in block_info["counts"]:                                   # BigGAN.py:624-664
                scope = 'resblock_down_' + str(ch_mul)
                for sb_i in range(block_count):
                    if block_count > 1:
                        scope = scope + '_' + str(sb_i)
                    if self.deep:                                                      # BigGAN.py:629-631
                        x = resblock_down_deep(x, channels_out=ch, use_bias=self.d_use_bias, opt=opt, scope=scope)
                        x = resblock_down_deep(x, channels_out=ch, downscale=False, use_bias=self.d_use_bias, opt=opt,
                                               scope=scope + "_2")
                    else:
                        x = resblock_down(x, channels=ch, use_bias=self.d_use_bias, opt=opt, scope=scope)
                b_i += 1
                if b_i == block_info["sa_index"]:
                    x = self_attention_2(x, channels=ch, opt=opt, scope='self_attention')
                if _recon is not None:                                                 # BigGAN.py:639-661
                    x = self._recon_heads(x, outputs, opt, _recon)
                ch = self.d_channels_for_block(b_i)
                ch_mul = ch_mul * 2
            ch = self.d_channels_for_block(b_i - 1)                                    # BigGAN.py:666
            x = resblock(x, channels=ch, use_bias=self.d_use_bias, opt=opt, scope='resblock')
            x = opt["act"](x)
            features = global_sum_pooling(x)                                           # BigGAN.py:671
            critic_opt = self.make_opt_with_sn(opt, self.d_compat_use_sn_in_critic_output)
            x = fully_connected(features, units=1, opt=critic_opt, scope='D_logit')    # BigGAN.py:681-682
            outputs["real"] = x
            if self.acgan:                                                             # BigGAN.py:686-701
                cls_opt = self.make_opt_with_sn(opt, self.d_compat_use_sn_in_classification)
                if self.args.d_cls_dense_layers:                                       # BigGAN.py:690-698
                    with S.variable_scope("classification"):
                        u1 = self.round_up(ch / 16.0 + self.n_labels * 1.25, 8)
                        y = fully_connected(features, units=u1, opt=cls_opt, scope='dense1')
                        y = opt["act"](y)
                        u2 = self.round_up(u1 / 4.0 + self.n_labels * 1.1, 4)
                        y = fully_connected(y, units=u2, opt=cls_opt, scope='dense2')
                        y = opt["act"](y)
                        y = fully_connected(y, units=self.n_labels, opt=cls_opt, scope='DC_logit')
                    outputs["cls"] = y
                else:
                    outputs["cls"] = fully_connected(features, units=self.n_labels, opt=cls_opt, scope='DC_logit')
            return outputs

    ##################################################################################
    # Model  (BigGAN.py:768-961)
    ##################################################################################
    def build_model(self):
        """Create every variable (one shape-only pass), pack trainables into flat arenas, set up the
        optimiser state (BigGAN.py:913-930: Adam for D; MovingAverageOptimizer(Adam) for G)."""
        B = 2
        z = torch.empty(B, 1, 1, self.z_dim, device="meta")
        img = self.generator(z, None, is_training=True)
        assert tuple(img.shape) == (B, self.img_size, self.img_size, self.c_dim), img.shape
        out = self.discriminator(img, _recon={"offsets": (None, None)} if self.recon_plan else None)
        assert tuple(out["real"].shape) == (B, 1)
        for key, head in (("coarse_logits", "coarse"), ("texture_logits", "texture")):
            if head in self.recon_plan:
                side = self.recon_plan[head].get("target") or self.recon_plan[head]["patch"]
                assert tuple(out[key].shape) == (B, side, side, self.c_dim), (key, out[key].shape)
        self.store.pack()
        self.g_arena = self.store.arenas["generator"]
        self.d_arena = self.store.arenas["discriminator"]
        self.d_vars = self.store.trainable_variables('discriminator')                  # BigGAN.py:915-917
        self.g_vars = self.store.trainable_variables('generator')
        self.sn_batches = {}
        if self.store.device.type == "cuda":
            # (the reconstruction heads run in one call of the D step only: their power iteration is a batch of its own,
            #  so that their ``u`` advances exactly when they run)
            def sn_group(name):
                if name.startswith("discriminator/upscaler/") or name.startswith("discriminator/tex_upscaler/"):
                    return "d_recon"
                return name.split("/", 1)[0]
            for group in ("generator", "discriminator", "d_recon"):
                arena = self.store.arenas["discriminator" if group == "d_recon" else group]
                names = [w for w, u in self.store.sn_pairs.items() if sn_group(w) == group and w in arena.offsets]
                pairs = [(self.store.vars[w], self.store.vars[self.store.sn_pairs[w]]) for w in names]
                for i in range(0, len(pairs), 256):
                    chunk = names[i:i + 256]
                    # f | g | h projections of every self-attention block share one packed GEMM operand
                    groups = []
                    for j, nm in enumerate(chunk):
                        if nm.endswith("/f_conv/kernel"):
                            pre = nm[:-len("f_conv/kernel")]
                            try:
                                groups.append([j, chunk.index(pre + "g_conv/kernel"), chunk.index(pre + "h_conv/kernel")])
                            except ValueError:
                                pass
                    # data parallelism: the power iteration is sharded by weight (SnBatch docstring; BG_SHARD_SN=0: replicated)
                    shard = None
                    if (self.world > 1 or os.environ.get("BG_SHARD_OPT", "") == "force") \
                            and os.environ.get("BG_SHARD_SN", "1") != "0" \
                            and torch.distributed.is_available() and torch.distributed.is_initialized():
                        shard = (self.rank, self.world, self.pg)
                    sb = Fn.SnBatch(pairs[i:i + 256], groups, shard)
                    if shard is not None:          # the u vectors now live in the batch's flat state buffer
                        for j, nm in enumerate(chunk):
                            self.store.vars[self.store.sn_pairs[nm]] = sb.u[j]
                    self.sn_batches.setdefault(group, []).append(sb)
        self.reg_owner = self._shard_regularisers()
        self._setup_exchange()
        self.counter = 0
        self.built = True
        return self

    def _setup_exchange(self):
        """Data parallelism: the process group of the large gradient / parameter exchanges (its own RCCL communicator
        and stream, parallel.new_gradient_group) and the STATIC partition of each arena into exchange ranges
        (parallel.ShardedRanges) - the generator's follow its stages, so that a stage's range can leave while backward
        is still running in the earlier stages; the discriminator's are 256 MiB chunks.  With --shard_optimizer (default
        under data parallelism; BG_SHARD_OPT=0 switches back to all-reduce + replicated update) every range is
        reduce-scattered, TF-Adam + EMA run on the owned 1/N and the parameters are all-gathered: Adam moments and EMA
        shadows then exist only on their owner (``sync_sharded_state`` assembles them for checkpoints and sampling)."""
        from .parallel import ShardedRanges, new_gradient_group
        self.pg_grad = None
        self._param_gathers = {"generator": [], "discriminator": []}
        self.shards = {}
        self.shard_opt = False
        force = os.environ.get("BG_SHARD_OPT", "") == "force"      # (tests: the sharded call sites on a 1-rank RCCL group)
        if (self.world == 1 and not force) or self.store.device.type != "cuda":
            return
        self.pg_grad = new_gradient_group(self.pg)
        self.shards["generator"] = ShardedRanges(self.g_arena.size, self._g_bucket_starts().values(), self.world, self.rank)
        self.shards["discriminator"] = ShardedRanges(self.d_arena.size, (), self.world, self.rank)
        want = os.environ.get("BG_SHARD_OPT", "1") != "0"
        self.shard_opt = want and (force or all(sh.sharded for sh in self.shards.values()))

    def _shard_regularisers(self):
        """The ortho-cosine terms depend on the weights only, so under data parallelism every rank would
        repeat the same 2 x 229 GFLOP (config 2) of Gram work.  Instead each kernel's term is evaluated
        on ONE rank (longest-processing-time assignment by GEMM cost) and the SUM all-reduce of the
        gradient arena delivers it everywhere."""
        if self.world == 1:
            return None
        cost = {}
        for name, shape in self.store.reg_shapes.items():
            c = shape[-1]
            rows = 1
            for d in shape[:-1]:
                rows *= d
            cost[name] = rows * rows * c if 2 * rows <= c else rows * c * c
        load = [0] * self.world
        owner = {}
        for name in sorted(cost, key=lambda k: (-cost[k], k)):
            r = min(range(self.world), key=lambda i: (load[i], i))
            owner[name] = r
            load[r] += cost[name]
        return owner

    def _begin_run(self):
        S.set_default_store(self.store)       # several models may live in one process: ops resolve variables here
        Fn.set_precision(self.precision)
        if getattr(self, "_zero_pool", None) is None and self.device.type == "cuda":
            self._zero_pool = Fn.ZeroPool(self.device)
        ops.begin_run(self._reduce_fn(), self.world, self.rank, getattr(self, "reg_owner", None),
                      getattr(self, "_zero_pool", None))

    def _sn_prefetch(self, group, x):
        if x.is_cuda:
            self._wait_params(group)          # (a sharded update's all-gather of this network may still be in flight)
            for b in getattr(self, "sn_batches", {}).get(group, ()):
                ops.sn_prefetch(b)

    def _sn_backward(self, group):
        for b in getattr(self, "sn_batches", {}).get(group, ()):
            b.backward()

    # ---- bucketed, overlapped exchange of the generator gradients (data parallel) -----------------------
    def _g_bucket_starts(self):
        """Arena offset at which the variables of each generator stage begin (stages in creation = arena order:
        first/*, resblock_up_<m> ..., [self_attention], ..., tail = batch_norm / prelu / G_logit)."""
        if getattr(self, "_g_starts", None) is None:
            arena = self.g_arena
            starts = {}
            for name in arena.names:
                off = arena.offsets[name][0]
                rest = name[len("generator/"):]
                top = rest.split("/")[0]
                if top.startswith("resblock_up_"):
                    key = "resblock_up_" + top[len("resblock_up_"):].split("_")[0]    # sub-blocks share their stage
                elif top in ("batch_norm", "prelu", "G_logit"):
                    key = "tail"
                else:
                    continue
                starts[key] = min(starts.get(key, off), off)
            self._g_starts = starts
        return self._g_starts

    def _grad_mark(self, x, tag):
        st = getattr(self, "_g_overlap", None)
        if st is None or not torch.is_grad_enabled() or not getattr(x, "requires_grad", False) or x.device.type != "cuda":
            return x
        y = Fn.GradMarkFn.apply(x, self._g_bucket_done, tag)
        sums = getattr(x, "bg_bn_sums", None)
        if sums is not None:
            y.bg_bn_sums = sums            # (fused batch-norm statistics of the block input travel with the marker's view)
        return y

    def _g_bucket_done(self, tag):
        """Backward has passed the input of stage ``tag``: every generator variable from that stage's first slot to the
        last not-yet-exchanged slot has its final gradient.  Turn dL/d(w/sigma) into dL/dw for the newly finished
        weights, zero what nothing wrote and start the asynchronous SUM all-reduce of that arena range."""
        st = self._g_overlap
        lo = self._g_bucket_starts().get(tag)
        if st is None or lo is None or lo >= st["hi"]:
            return
        self._g_exchange_range(lo, st["hi"])
        st["hi"] = lo

    def _g_exchange_range(self, lo, hi):
        st = self._g_overlap
        self._sn_backward("generator")                      # (only the weights touched since the last call)
        self.store.zero_untouched("generator", lo, hi)
        st["handles"].extend(self._exchange_begin("generator", lo, hi, st["apply"]))

    # ---- data-parallel hooks -----------------------------------------------------------------
    def _reduce_fn(self):
        if self.world == 1:
            return None
        pg = self.pg

        def red(t):
            torch.distributed.all_reduce(t, group=pg)
        return red

    def _exchange_begin(self, group, lo, hi, apply, async_op=True):
        """Start the exchange of the gradient ranges inside [lo, hi) of an arena on the gradient process group:
        reduce-scatter when the update that follows is sharded (each rank then holds the summed gradient of the part it
        owns), all-reduce otherwise (``apply`` False: callers that want the whole summed gradient; or sharding is off).
        Returns handles for ``_exchange_end``."""
        from .parallel import reduce_scatter_range
        arena = self.store.arenas[group]
        sh = self.shards[group]
        pg = self.pg_grad if self.pg_grad is not None else self.pg
        out = []
        for a, b in sh.containing(lo, hi):
            if self.shard_opt and apply:
                w = reduce_scatter_range(arena.grads, a, b, sh, pg, async_op=async_op)
                out.append((a, b, w, True))
            else:
                w = torch.distributed.all_reduce(arena.grads.narrow(0, a, b - a), group=pg, async_op=async_op)
                out.append((a, b, w, False))
        return out

    def _exchange_end(self, group, handles, lr, with_ema, apply, grad_scale=1.0):
        """Wait for each exchanged range in issue order and update it: TF-Adam (+ EMA) on the owned part followed by the
        asynchronous all-gather of the new parameters (sharded), or on the whole range (replicated).  The all-gathers
        are waited for by the first reader of that network's parameters (``_wait_params``)."""
        from .parallel import all_gather_range
        arena = self.store.arenas[group]
        sh = self.shards[group]
        pg = self.pg_grad if self.pg_grad is not None else self.pg
        for a, b, work, scattered in handles:
            if work is not None:
                work.wait()
            if not apply:
                continue
            if scattered:
                oa, ob = sh.owned(a, b)
                self._adam(arena, lr, with_ema=with_ema, grad_scale=grad_scale, lo=oa, hi=ob, prepare=False)
                self._param_gathers[group].append(all_gather_range(arena.params, a, b, sh, pg, async_op=True))
            else:
                self._adam(arena, lr, with_ema=with_ema, grad_scale=grad_scale, lo=a, hi=b, prepare=False)

    def _wait_params(self, group=None):
        """Block the compute stream until the parameters of a network are whole again after a sharded update."""
        for g in ((group,) if group else tuple(getattr(self, "_param_gathers", {}))):
            works = self._param_gathers.get(g, ())
            for w in works:
                w.wait()
            if works:
                del works[:]

    def sync_sharded_state(self):
        """Assemble the optimiser state that a sharded update keeps only on its owner - Adam m / v and the generator's EMA
        shadows - on every rank (all-gather per exchange range).  Collective: every rank calls it (checkpoints, sampling
        with the EMA weights, state comparisons in tests)."""
        self._wait_params()
        if not getattr(self, "shard_opt", False):
            return
        from .parallel import all_gather_range
        for group, sh in self.shards.items():
            arena = self.store.arenas[group]
            for buf in (arena.m, arena.v, arena.ema):
                if buf is None:
                    continue
                for a, b in sh.ranges:
                    all_gather_range(buf, a, b, sh, self.pg_grad)

    def _adam_prepare(self, arena, lr):
        """Host part of an optimiser step: advance the step count and put the bias-corrected step size
        lr * sqrt(1 - beta2^t) / (1 - beta1^t) (tf.train.AdamOptimizer) into the arena's device scalar."""
        arena.step += 1
        t = arena.step
        lr_t = lr * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)
        if getattr(arena, "lr_dev", None) is None:
            arena.lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        arena.lr_dev.fill_(lr_t)

    def _adam(self, arena, lr, with_ema, grad_scale=1.0, lo=0, hi=None, prepare=True):
        """TF-Adam (+ EMA) on the arena, or on its slice [lo, hi) (the optimiser is elementwise)."""
        if prepare and not getattr(self, "_capturing", False):
            self._adam_prepare(arena, lr)          # (a captured graph is replayed after _adam_prepare on the host)
        hi = arena.size if hi is None else hi
        sl = (lambda t: t.narrow(0, lo, hi - lo)) if (lo, hi) != (0, arena.size) else (lambda t: t)
        hip.check(hip.lib().bg_adam_tf_ema_step_dev(
            hip.f32(sl(arena.params)), hip.f32(sl(arena.grads)), hip.f32(sl(arena.m)), hip.f32(sl(arena.v)),
            hip.f32(sl(arena.ema)) if with_ema else None, hip.f32(arena.lr_dev), self.beta1, self.beta2, 1e-8,
            self.moving_decay, float(grad_scale), hi - lo, hip.stream()))

    def sample_z(self, B):
        z = torch.empty(B, 1, 1, self.z_dim, dtype=torch.float32, device=self.device)
        if self.z_trunc_train:                                                         # BigGAN.py:790-793
            torch.nn.init.trunc_normal_(z, 0.0, 1.0, -2.0, 2.0, generator=self.gen)
        else:
            z.normal_(generator=self.gen)
        return z

    def _set_requires_grad(self, variables, flag):
        for v in variables.values():
            v.requires_grad_(flag)

    # ---- the two train ops -------------------------------------------------------------------------
    def _cls_loss(self):
        if getattr(self, "_cls_loss_fn", None) is None:
            w = torch.tensor(self.cls_loss_weights, dtype=torch.float32, device=self.device)
            self._cls_loss_fn = cls_loss_fn(self.cls_loss_type, w)                     # BigGAN.py:851-852
        return self._cls_loss_fn

    def gp_draws(self, B):
        """The random inputs of one gradient_penalty() call (BigGAN.py:719, 726, 729): eps ~ U[0,1) with the
        batch's shape (dragan only), alpha ~ U[0,1) per sample, and one set of DiffAugment draws."""
        from .DiffAugment import draw
        S_ = self.img_size
        out = {"alpha": torch.rand(B, dtype=torch.float32, device=self.device, generator=self.gen),
               "aug": draw(B, S_, self.device, self.gen) if self.da_policy else None}
        if self.gradient_penalty_type == 'dragan':
            out["eps"] = torch.rand(B, S_, S_, self.c_dim, dtype=torch.float32, device=self.device, generator=self.gen)
        return out

    def gradient_penalty(self, real, fake, draws=None):
        """BigGAN.py:717-742.  GP = ld * mean phi(||d D(aug(x^))/d x^||) on x^ between the real batch and the fake
        batch (wgan-gp / wgan-lp) or a perturbed real batch (dragan).  Three discriminator passes on x^:
        (1) forward + an inputs-only backward give g = dD/dx^, its norms, the penalty's value and the constant
        direction v = ld * phi'(||g||)/count * g/||g||;  (2) a forward-mode pass carries (x^, v) through DiffAugment
        and D as a ``Dual`` and yields the directional derivatives fdot = <g(theta), v>;  (3) the ordinary backward
        of d_loss differentiates fdot w.r.t. the parameters, which IS d GP/d theta (v held constant)."""
        from .ops import Dual
        L = Fn.lib()
        B = real.shape[0]
        per = real.numel() // B
        if draws is None:
            draws = self.gp_draws(B)
        real = real.contiguous()
        xhat = torch.empty_like(real)
        if self.gradient_penalty_type == 'dragan':
            sums = torch.zeros(2, dtype=torch.float64, device=self.device)
            Fn.check(L.bg_bn_stats_t(Fn.f32(real), Fn.hip.F32, Fn.hip.ptr(sums), real.numel(), 1, Fn.stream()))
            if self._reduce_fn() is not None:          # the moments of the GLOBAL real batch (BigGAN.py:720)
                self._reduce_fn()(sums)
            Fn.check(L.bg_gp_interpolate(Fn.f32(real), Fn.f32(draws["eps"].contiguous()), Fn.f32(draws["alpha"]),
                                         Fn.hip.ptr(sums), float(real.numel() * self.world), Fn.f32(xhat), B, per,
                                         Fn.stream()))
        else:
            Fn.check(L.bg_gp_interpolate(Fn.f32(real), Fn.f32(fake.detach().contiguous()), Fn.f32(draws["alpha"]), None,
                                         0.0, Fn.f32(xhat), B, per, Fn.stream()))
        aug = draws.get("aug")
        if Fn.Precision.resident:          # bf16-resident model: the penalty's passes run on fp32 tensors (bf16 MFMA)
            with Fn.precision_scope("bf16-staged"):
                return self._gradient_penalty_passes(xhat, draws, aug, B, per)
        return self._gradient_penalty_passes(xhat, draws, aug, B, per)

    def _gradient_penalty_passes(self, xhat, draws, aug, B, per):
        from .ops import Dual
        L = Fn.lib()
        # (1) g = d sum(D(aug(x^))) / d x^
        xg = xhat.detach().requires_grad_(True)
        logit = self.discriminator(DiffAugment(xg, policy=self.da_policy, draws=aug), reuse=True)["real"]
        seed = torch.empty_like(logit)
        seed.fill_(1.0)
        with Fn.inputs_only_backward():
            g, = torch.autograd.grad(logit, xg, grad_outputs=seed)
        g = g.contiguous()
        ws = torch.empty(2 * B, dtype=torch.float64, device=self.device)
        value = torch.empty(1, dtype=torch.float32, device=self.device)
        v = torch.empty_like(g)
        Fn.check(L.bg_gp_penalty(Fn.f32(g), B, per, float(B * self.world), float(self.ld),
                                 int(self.gradient_penalty_type == 'wgan-lp'), Fn.hip.ptr(ws), Fn.f32(value), Fn.f32(v),
                                 Fn.stream()))
        red = self._reduce_fn()
        if red is not None:
            red(value)
        # (2) forward-mode pass; the tangent of DiffAugment is DiffAugment without the brightness offset
        if self.da_policy:
            lin = dict(aug)
            lin["u_b"] = torch.full_like(aug["u_b"], 0.5)
            dual = Dual(DiffAugment(xhat, policy=self.da_policy, draws=aug),
                        DiffAugment(v, policy=self.da_policy, draws=lin))
        else:
            dual = Dual(xhat, v)
        fdot = self.discriminator(dual, reuse=True)["real"].t
        return Fn.GpSurrogateFn.apply(fdot, value)

    def d_forward(self, real, z=None, draws_real=None, draws_fake=None, labels=None, cls_z=None, gp_draws=None,
                  recon_offsets=None):
        """BigGAN.py:806-808, 856-883: D(aug(real)), D(aug(G(z))), hinge + flood (+ the label loss on the
        real half when n_labels > 0, BigGAN.py:853).  G runs without a backward graph (d_loss is minimised
        over d_vars only); real and fake go through D as one batch.  With a reconstruction head (BigGAN.py:810-836,
        885-889) the real batch takes a call of its own, the only one the heads run in; ``recon_offsets``: explicit
        (ro_x, ro_y) int32 device tensors of the texture crop (drawn when None)."""
        B = real.shape[0]
        self._begin_run()
        if z is None:
            z = self.sample_z(B)
        if self.acgan and cls_z is None:
            cls_z = self.draw_labels(B)                                                # rnd_cls_feed_dict, BigGAN.py:1454
        with torch.no_grad():
            fake = self.generator(z, cls_z, is_training=True)
        real_aug = DiffAugment(real, policy=self.da_policy, draws=draws_real, generator=self.gen)
        fake_aug = DiffAugment(fake, policy=self.da_policy, draws=draws_fake, generator=self.gen)
        recon = None
        if self.recon_plan:
            recon = {"offsets": (None, None)}
            if "texture" in self.recon_plan:
                tp = self.recon_plan["texture"]
                recon["offsets"] = recon_offsets if recon_offsets is not None else \
                    self.random_crop_offsets((B, tp["size"], tp["size"]), tp["feat_patch"])
        if self.bn_in_d or recon is not None:
            # batch norm couples the samples of a call: keep the reference's two instantiations
            # (BigGAN.py:807,857), each with its own batch statistics; moving statistics compound
            d_real = self.discriminator(real_aug, _recon=recon)
            d_fake = self.discriminator(fake_aug, reuse=True)
            real_logits, fake_logits = d_real["real"], d_fake["real"]
            d_out = d_real
        else:
            d_out = self.discriminator(torch.cat([real_aug, fake_aug], dim=0))
            logits = d_out["real"]
            real_logits, fake_logits = logits[:B], logits[B:]
        d_loss = discriminator_loss(self.d_loss_func, real=real_logits, fake=fake_logits, flood_level=self.d_flood)
        out = {"real_logits": real_logits, "fake_logits": fake_logits, "fake": fake}
        if self.use_gradient_penalty:                                                  # BigGAN.py:867-868, 880
            out["gp"] = self.gradient_penalty(real, fake, gp_draws)
            d_loss = Fn.AddFn.apply(d_loss, out["gp"])
        if self.acgan:
            if labels is None:
                raise ValueError("n_labels > 0: d_forward needs the labels of the real batch")
            out["cls_z"] = cls_z                    # the generator's labels of this run (drawn or given)
            real_cls = d_out["cls"][:B]             # (a no-op slice when D ran on the real batch alone)
            d_cls = self._cls_loss()(labels, real_cls, self.d_cls_loss_weight, self._reduce_fn(), self.world)
            out["d_cls_loss"] = d_cls
            d_loss = Fn.AddFn.apply(d_loss, d_cls)
        if recon is not None:                                                          # BigGAN.py:810-836, 885-889
            red, ro_x, ro_y = self._reduce_fn(), recon["offsets"][0], recon["offsets"][1]
            if "coarse" in self.recon_plan:
                mode = Fn.RECON_HALFRES if self.d_reconstruction_halfres else Fn.RECON_IDENTITY
                out["d_recon"], out["coarse_upscaled"] = Fn.ReconLossFn.apply(
                    d_real["coarse_logits"], real_aug, None, None, mode, 1, self.d_recon_ld, red, self.world)
                d_loss = Fn.AddFn.apply(d_loss, out["d_recon"])
            if "texture" in self.recon_plan:
                out["d_tex_recon"], out["texture_upscaled"] = Fn.ReconLossFn.apply(
                    d_real["texture_logits"], real_aug, ro_x, ro_y, Fn.RECON_CROP, self.recon_plan["texture"]["f"],
                    self.d_tex_recon_ld, red, self.world)
                d_loss = Fn.AddFn.apply(d_loss, out["d_tex_recon"])
                out["rnd_offset_x"], out["rnd_offset_y"] = ro_x, ro_y
            out["real_aug"] = real_aug
        out["d_loss"] = d_loss
        return out

    def _per_virtual_batch(self, k, v):
        if isinstance(v, (list, tuple)):
            if len(v) != self.virtual_batches:
                raise ValueError("expected %d virtual batches, got %d" % (self.virtual_batches, len(v)))
            return v[k]
        return v

    def _recon_offsets_for(self, k, v):
        """One (ro_x, ro_y) pair for every virtual batch, or a list of --virtual_batches pairs."""
        if v is not None and isinstance(v[0], (list, tuple)):
            return self._per_virtual_batch(k, list(v))
        return v

    def d_step(self, real, z=None, draws_real=None, draws_fake=None, apply=True, labels=None, cls_z=None,
               defer=False, gp_draws=None, recon_offsets=None):
        """One run of d_ops (utils.py:252-320): with --virtual_batches k, gradients of k forward/backward
        passes (each on its own real batch / z / draws; lists of k are accepted) are accumulated and
        applied once, scaled 1/k; reported losses are means over the k passes."""
        vb = self.virtual_batches
        self.store.begin_backward("discriminator")
        outs = []
        for k in range(vb):
            out = self.d_forward(*[self._per_virtual_batch(k, a) for a in (real, z, draws_real, draws_fake, labels)],
                                 cls_z=cls_z,                                        # one feed_dict for all k
                                 gp_draws=self._per_virtual_batch(k, gp_draws),
                                 recon_offsets=self._recon_offsets_for(k, recon_offsets))
            out["d_loss"].backward()
            self._sn_backward("discriminator")
            self._sn_backward("d_recon")
            outs.append(out)
        self.store.zero_untouched("discriminator")
        if self.shards:
            # data parallel: start the exchange of the D gradients (reduce-scatter, or all-reduce when the update is
            # replicated); with ``defer`` return at once - the generator forward of the G step does not read D, so it
            # runs while the collectives are in flight, and _finish_d() (wait, Adam on the owned part, all-gather of
            # the parameters) is called just before the G step's first use of the discriminator
            handles = self._exchange_begin("discriminator", 0, self.d_arena.size, apply)
            self._pending_d = (handles, bool(apply), 1.0 / vb)
            if not defer:
                self._finish_d()
        elif apply:
            self._adam(self.d_arena, self.d_learning_rate, with_ema=False, grad_scale=1.0 / vb)
        return self._mean_losses(outs, ("d_loss", "d_cls_loss", "gp", "d_recon", "d_tex_recon"))

    def _finish_d(self):
        pending = getattr(self, "_pending_d", None)
        if pending is None:
            return
        handles, apply, gscale = pending
        self._pending_d = None
        if apply:
            self._adam_prepare(self.d_arena, self.d_learning_rate)
        self._exchange_end("discriminator", handles, self.d_learning_rate, False, apply, gscale)

    def _mean_losses(self, outs, keys):
        out = outs[-1]
        if len(outs) > 1:
            for key in keys:
                if key in out and out[key] is not None:
                    acc = outs[0][key].detach().clone()
                    for o in outs[1:]:
                        Fn.axpby(o[key].detach(), 1.0, acc, 1.0)
                    out[key] = Fn.axpby(acc, 0.0, acc, 1.0 / len(outs))
        return out

    def g_forward(self, B, z=None, draws_fake=None, cls_z=None, after_generator=None, real=None, draws_real=None):
        """BigGAN.py:896-898: -mean(D(aug(G(z)))) + flood (+ label loss, BigGAN.py:894) + regularisation losses."""
        self._begin_run()
        if z is None:
            z = self.sample_z(B)
        if self.acgan and cls_z is None:
            cls_z = self.draw_labels(B)
        fake = self.generator(z, cls_z, is_training=True)
        if after_generator is not None:
            after_generator()               # e.g. the deferred D update: must precede any use of the discriminator
        fake_aug = DiffAugment(fake, policy=self.da_policy, draws=draws_fake, generator=self.gen)
        real_logits = None
        if self.relativistic:
            # g_loss of the ra-* types reads D(aug(real)) too (BigGAN.py:806-808, 896); D's weights are frozen
            # in this op, so the real half needs no backward graph
            if real is None:
                raise ValueError("--gan_type %s: the G step needs a real batch" % self.gan_type)
            real_aug = DiffAugment(real, policy=self.da_policy, draws=draws_real, generator=self.gen)
            if self.bn_in_d:
                real_logits = self.discriminator(real_aug)["real"]
                d_out = self.discriminator(fake_aug, reuse=True)
                fake_logits = d_out["real"]
            else:
                d_out = self.discriminator(torch.cat([real_aug, fake_aug], dim=0))
                nr = real_aug.shape[0]
                real_logits, fake_logits = d_out["real"][:nr], d_out["real"][nr:]
                if self.acgan:
                    d_out = dict(d_out, cls=d_out["cls"][nr:])
        else:
            d_out = self.discriminator(fake_aug)
            fake_logits = d_out["real"]
        g_adv = generator_loss(self.gan_type, fake=fake_logits, real=real_logits, flood_level=self.g_flood)
        out = {"fake_logits": fake_logits, "fake": fake}
        if self.acgan:
            g_cls = self._cls_loss()(cls_z, d_out["cls"], self.g_cls_loss_weight, self._reduce_fn(), self.world)
            out["g_cls_loss"] = g_cls
            out["cls_z"] = cls_z
            g_adv = Fn.AddFn.apply(g_adv, g_cls)
        out["g_adv"] = g_adv
        out["regs"] = ops.get_regularization_losses() if self.g_regularization_method != 'none' else []
        return out

    def g_step(self, B, z=None, draws_fake=None, apply=True, cls_z=None, after_generator=None, real=None,
               draws_real=None):
        vb = self.virtual_batches
        self._set_requires_grad(self.d_vars, False)        # g_loss is minimised over g_vars only
        outs = []
        # data parallel: exchange the generator gradients stage by stage while backward is still running
        overlap = (vb == 1 and self.device.type == "cuda" and bool(getattr(self, "shards", None))
                   and not getattr(self, "_capturing", False))
        self._g_overlap = {"hi": self.g_arena.size, "handles": [], "apply": bool(apply)} if overlap else None
        try:
            self.store.begin_backward("generator")
            for k in range(vb):
                out = self.g_forward(B, self._per_virtual_batch(k, z), self._per_virtual_batch(k, draws_fake), cls_z,
                                     after_generator if k == 0 else None, self._per_virtual_batch(k, real),
                                     self._per_virtual_batch(k, draws_real))
                roots = [out["g_adv"]] + out["regs"]
                ones = torch.ones(1, dtype=torch.float32, device=self.device)
                # each regularisation term is evaluated on exactly one rank (_shard_regularisers): weight 1,
                # the SUM all-reduce of the flat gradient arena then yields the single-process gradient
                torch.autograd.backward(roots, [ones] * len(roots))
                self._sn_backward("generator")
                out["g_reg"] = Fn.zeros(1, torch.float32, self.device)
                if out["regs"]:                                     # reported value: column sum of the terms
                    terms = torch.cat([r.detach().reshape(1) for r in out["regs"]]).reshape(-1, 1)
                    Fn._bias_grad(terms, out["g_reg"])
                if self.world > 1 and self.g_regularization_method != 'none':
                    self._reduce_fn()(out["g_reg"])                 # sum over the owners
                out["g_loss"] = Fn.axpby(out["g_reg"], 1.0, out["g_adv"].detach().clone().reshape(1), 1.0)
                outs.append(out)
        finally:
            self._set_requires_grad(self.d_vars, True)
            st, self._g_overlap = getattr(self, "_g_overlap", None), None
        if st is not None:
            self._g_overlap = st
            if st["hi"] > 0:
                self._g_exchange_range(0, st["hi"])         # first/* (and anything no marker covered)
            self._g_overlap = None
            if apply:
                self._adam_prepare(self.g_arena, self.g_learning_rate)
            # in completion order: the last exchange overlaps the optimiser (and the all-gathers) of the earlier ranges
            self._exchange_end("generator", st["handles"], self.g_learning_rate, True, apply, 1.0)
            return self._mean_losses(outs, ("g_adv", "g_reg", "g_loss", "g_cls_loss"))
        self.store.zero_untouched("generator")
        if self.shards:
            handles = self._exchange_begin("generator", 0, self.g_arena.size, apply)
            if apply:
                self._adam_prepare(self.g_arena, self.g_learning_rate)
            self._exchange_end("generator", handles, self.g_learning_rate, True, apply, 1.0 / vb)
        elif apply:
            self._adam(self.g_arena, self.g_learning_rate, with_ema=True, grad_scale=1.0 / vb)
        return self._mean_losses(outs, ("g_adv", "g_reg", "g_loss", "g_cls_loss"))

    def train_step(self, real, labels=None, real_g=None):
        """One iteration of BigGAN.py:1061-1084.  ``real`` (and ``labels`` when n_labels > 0) may be lists
        of --virtual_batches tensors.  ``real_g``: the real batch of the G op - the reference's g_ops pull a FRESH
        batch from the input iterator (BigGAN.py:1082), which matters for the relativistic losses whose generator
        loss reads D(real); None re-uses the D op's batch.  After ``capture_graphs()`` the iteration is replayed
        from HIP graphs."""
        if getattr(self, "_graphs_ready", False):
            if self.acgan and labels is None:
                labels = self.synthetic_labels(real.shape[0])
            return self._train_step_graph(real, labels, real_g)
        return self._train_step_eager(real, labels, real_g)

    def _train_step_eager(self, real, labels=None, real_g=None):
        losses = {}
        first = real[0] if isinstance(real, (list, tuple)) else real
        if self.acgan and labels is None:
            labels = [self.synthetic_labels(first.shape[0]) for _ in range(self.virtual_batches)]
        run_g = (self.counter - 1) % self.n_critic == 0                               # BigGAN.py:1080
        d = self.d_step(real, labels=labels, defer=run_g)
        losses["d_loss"] = d["d_loss"]
        if d.get("gp") is not None:
            losses["gp"] = d["gp"]
        for key in ("d_recon", "d_tex_recon"):
            if key in d:
                losses[key] = d[key]
        self._last_d_out = d if self.d_save_recon_samples else None
        if run_g:
            g = self.g_step(first.shape[0], after_generator=self._finish_d,
                            real=(real_g if real_g is not None else real) if self.relativistic else None)
            losses["g_loss"] = g["g_loss"]
        self._finish_d()
        self.counter += 1
        return losses

    # ---- HIP-graph replay of the iteration (launch-bound configurations) -------------------------
    def capture_graphs(self, B=None):
        """Capture the D op and the G op (forward, backward, spectral-norm batches, optimiser) into two HIP
        graphs (torch.cuda.CUDAGraph) with static input buffers.  ``train_step`` then copies the batch in,
        refreshes the two Adam step sizes on the host and replays: ~4000 kernel launches per iteration cost
        two graph launches, which is what bounds small configurations (BASELINE config 1 spends 6 ms of a
        16 ms step in kernels).  Single process only (collectives are not captured)."""
        if self.world != 1:
            raise NotImplementedError("graph capture is for single-process runs")
        if self.virtual_batches != 1:
            raise NotImplementedError("graph capture with --virtual_batches > 1")
        B = B or self.batch_size
        self._g_real = torch.zeros(B, self.img_size, self.img_size, self.c_dim, dtype=torch.float32, device=self.device)
        self._g_labels = (torch.zeros(B, self.n_labels, dtype=torch.float32, device=self.device) if self.acgan else None)
        self._g_real_g = torch.zeros_like(self._g_real) if self.relativistic else None     # the G op's own real batch
        if getattr(self.d_arena, "lr_dev", None) is None:
            for arena in (self.d_arena, self.g_arena):
                arena.lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        # untimed eager warm-up on a side stream (allocator pools, lazy initialisation), state restored afterwards
        snap = self.state_tensors()
        saved = {k: v.detach().clone() for k, v in snap.items()}
        steps = (self.counter, self.d_arena.step, self.g_arena.step)
        rng = self.gen.get_state()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._train_step_eager(self._g_real, self._g_labels)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

        def restore():
            with torch.no_grad():
                for k, v in snap.items():
                    v.copy_(saved[k])
            self.counter, self.d_arena.step, self.g_arena.step = steps
            self.gen.set_state(rng)
        restore()
        self._capturing = True
        try:
            self._graph_d = torch.cuda.CUDAGraph()
            self._graph_d.register_generator_state(self.gen)
            with torch.cuda.graph(self._graph_d):
                self._g_out_d = self.d_step(self._g_real, labels=self._g_labels)
            self._graph_g = torch.cuda.CUDAGraph()
            self._graph_g.register_generator_state(self.gen)
            with torch.cuda.graph(self._graph_g, pool=self._graph_d.pool()):
                self._g_out_g = self.g_step(B, real=self._g_real_g if self.relativistic else None)
        finally:
            self._capturing = False
        torch.cuda.synchronize()
        restore()                      # capture does not execute kernels, but it advanced host-side bookkeeping
        self._graphs_ready = True
        return self

    def _train_step_graph(self, real, labels, real_g=None):
        self._g_real.copy_(real)
        if self._g_real_g is not None:
            self._g_real_g.copy_(real_g if real_g is not None else real)
        if self._g_labels is not None:
            self._g_labels.copy_(labels)
        losses = {}
        self._adam_prepare(self.d_arena, self.d_learning_rate)
        self._graph_d.replay()
        losses["d_loss"] = self._g_out_d["d_loss"]
        for key in ("d_recon", "d_tex_recon"):
            if key in self._g_out_d:
                losses[key] = self._g_out_d[key]
        self._last_d_out = self._g_out_d if self.d_save_recon_samples else None
        if (self.counter - 1) % self.n_critic == 0:
            self._adam_prepare(self.g_arena, self.g_learning_rate)
            self._graph_g.replay()
            losses["g_loss"] = self._g_out_g["g_loss"]
        self.counter += 1
        return losses

    def synthetic_labels(self, B):
        """Synthetic one-hot labels, uniform classes: the labels of a run without a label file (with one, the reference
        draws tags from it, BigGAN.py:1446-1455, and so does ``draw_labels``)."""
        idx = torch.randint(0, self.n_labels, (B,), device=self.device, generator=self.gen)
        lab = torch.zeros(B, self.n_labels, dtype=torch.float32, device=self.device)
        lab[torch.arange(B, device=self.device), idx] = 1.0
        return lab

    def draw_labels(self, B):
        """The generator's labels of one run of d_ops / g_ops (rnd_cls_feed_dict, BigGAN.py:1447-1455): ``B`` rows drawn
        with replacement from the dataset's label table, on the device (randint on ``self.gen`` + bg_gather_rows: both are
        captured, so a replayed graph draws fresh rows).  Without a table (synthetic data): ``synthetic_labels``."""
        if self.label_table is None:
            return self.synthetic_labels(B)
        idx = torch.randint(0, self.label_table.shape[0], (B,), device=self.device, generator=self.gen)
        return Fn.gather_rows(self.label_table, idx)

    def synthetic_batch(self, B=None):
        """Synthetic images U(-1,1) [B,S,S,c_dim] on the device (the reference reads PNG files)."""
        B = B or self.batch_size
        return torch.rand(B, self.img_size, self.img_size, self.c_dim, device=self.device,
                          generator=self.gen) * 2.0 - 1.0

    @staticmethod
    def settle_host():
        """Take the long-lived object graph (variables, arenas, autograd Function classes, ctypes tables: hundreds of
        thousands of objects) out of Python's cyclic garbage collector: a generation-2 collection that has to traverse it
        stalls the enqueueing thread for 45-75 ms (measured r02 at iteration 6 of a config-3 run, tools/host_time.py) -
        under data parallelism every rank waits for the stalled one.  Call after build_model() (and a first iteration)."""
        import gc
        gc.collect()
        gc.freeze()

    def train(self, data_fn=None, iterations=None, resume=True, samples=False):
        """BigGAN.py:1015-1118 training loop (synthetic data unless ``data_fn`` is given): resume from the
        latest checkpoint of ``checkpoint_dir`` if there is one, print the losses every iteration, save
        every ``save_freq`` iterations of an epoch (rank 0 writes; replicas are identical).  ``samples``: write the
        sample grids of ``save_samples`` every ``print_freq`` iterations of an epoch (BigGAN.py:1125; the command line
        turns it on, programmatic callers opt in).  With ``self.log_events`` set (the command line sets it, programmatic
        callers opt in) rank 0 writes a TensorBoard event file under ``<log_dir>/<model_dir>/`` (BigGAN.py:1019): every
        loss as a scalar each iteration and, every ``histogram_freq`` iterations, a histogram of every variable
        (trainlog.py)."""
        loader = None
        if data_fn is None:
            loader = self.open_dataset()
            if loader is not None:
                data_fn = lambda: next(loader)                                    # noqa: E731
        try:
            return self._train_loop(data_fn, iterations, resume, samples, bool(getattr(self, "log_events", False)))
        finally:
            self._close_log()
            if loader is not None:
                loader.close()

    def open_dataset(self, root="./dataset", device_preprocess=None, cache_bytes=None):
        """BigGAN.py:195-212, 768-787: the files of ``<root>/<--dataset>/`` (+ ``--label_file``) behind the
        reference's shuffle / decode / resize / flip / batch pipeline; None when that folder does not exist
        (the training loop then runs on synthetic batches).  ``device_preprocess``: BatchLoader's switch (None: resize,
        flip and normalise on the GPU unless BG_DEVICE_INPUT=0).  ``cache_bytes``: BatchLoader's budget of the
        device-resident dataset (None: BG_DEVICE_DATASET_GB; 0: off)."""
        from . import data as D
        folder = os.path.join(root, self.dataset_name)
        if not os.path.isdir(folder):
            return None
        files, labels = D.load_data(self.dataset_name, self.args.label_file, self.args.weight_file,
                                    ignore_missing=self.args.ignore_missing_labels, n_labels=self.n_labels, root=root)
        if self.acgan and labels is None:
            raise ValueError("--n_labels > 0 needs --label_file")
        if self.acgan:
            for path, row in zip(files, labels):
                if len(row) != self.n_labels:
                    raise ValueError("label file %s: %s has %d labels, --n_labels is %d"
                                     % (self.args.label_file, os.path.basename(path), len(row), self.n_labels))
        self.labels = labels if self.acgan else None          # (the sampler draws its class vectors from these rows)
        # ... and so does every training run of G, on the device (draw_labels)
        # (one fp32 row per listed file, so --weight_file's copies repeat their row, as in the reference's self.labels)
        self.label_table = None
        if self.acgan:
            import numpy as np
            self.label_table = torch.from_numpy(np.asarray(labels, dtype=np.float32).reshape(len(labels), self.n_labels)
                                                ).to(self.device)
        print("# dataset number:", len(files))
        image_data = D.ImageData(self.img_size, self.c_dim, True, self.args.random_flip, seed=1234 + self.rank)
        return D.BatchLoader(files, labels if self.acgan else None, self.batch_size, image_data, self.device,
                             seed=4321, rank=self.rank, world=self.world, device_preprocess=device_preprocess,
                             cache_bytes=cache_bytes)

    def _open_log(self):
        """A new event file per run, resumed runs included (tf.summary.FileWriter, BigGAN.py:1019).  Rank 0 only: replicas
        are identical, and the histogram kernel involves no collective."""
        from . import trainlog
        self._log_writer = trainlog.EventWriter(os.path.join(self.log_dir, self.model_dir))
        self._log_hists = trainlog.VariableHistograms(self.store, self.device) if self.histogram_freq else None

    def _close_log(self):
        writer = getattr(self, "_log_writer", None)
        self._log_writer = self._log_hists = None
        if writer is not None:
            writer.close()

    def _log_iteration(self, vals):
        """Summaries of the iteration that just ran; its step is the reference's counter before the increment.  Reads
        variables and the losses already fetched: no draw from ``self.gen``, nothing written, outside the HIP graphs."""
        step = self.counter - 1
        self._log_writer.add_scalars(step, vals)                                       # utils.py:291-294
        if self._log_hists is not None and step % self.histogram_freq == 0:           # BigGAN.py:1100-1101
            self._wait_params()               # (sharded update: the all-gather of the new parameters may be in flight)
            self._log_writer.add_histograms(step, self._log_hists.compute())
        if self.counter % self.print_freq == 0:
            self._log_writer.flush()

    def _train_loop(self, data_fn, iterations, resume, samples=False, log=False):
        could_load, checkpoint_counter = (self.load(self.checkpoint_dir) if resume else (False, 0))
        self._log_writer = self._log_hists = None
        if log and self.rank == 0:
            self._open_log()
        if could_load:
            start_epoch = int(checkpoint_counter / self.iterations_per_epoch)
            start_batch_id = checkpoint_counter - start_epoch * self.iterations_per_epoch
            print(" [*] Load SUCCESS")
        else:
            start_epoch, start_batch_id = 0, 0
            if resume:
                print(" [!] Load failed...")
        start_time = time.time()
        done = 0
        self.settle_host()
        for epoch in range(start_epoch, self.epoch):
            for idx in range(start_batch_id, self.iterations_per_epoch):
                if iterations is not None and done >= iterations:
                    return
                batch = data_fn() if data_fn is not None else self.synthetic_batch()
                real_g = None
                if self.relativistic and (self.counter - 1) % self.n_critic == 0:  # g_ops take their own batch (BigGAN.py:1082)
                    nxt = data_fn() if data_fn is not None else self.synthetic_batch()
                    real_g = nxt[0] if isinstance(nxt, tuple) else nxt
                if isinstance(batch, tuple):                                       # (images, labels) with --n_labels
                    losses = self.train_step(batch[0], labels=batch[1], real_g=real_g)
                else:
                    losses = self.train_step(batch, real_g=real_g)
                done += 1
                vals = {k: float(v.item()) for k, v in losses.items()}
                print_str = "Step: %5d, time: %4.4f" % (self.counter, time.time() - start_time)   # BigGAN.py:1109-1116
                for name, val in vals.items():
                    print_str += ", " + name + ": %.4f" % val
                if self.rank == 0:
                    print(print_str, flush=True)
                if self._log_writer is not None:
                    self._log_iteration(vals)
                if self.d_save_recon_samples and self.counter % self.print_freq == 0 and self.rank == 0:
                    self.save_recon_samples(epoch, idx + 1)                            # BigGAN.py:1050-1074
                if (idx + 1) % self.save_freq == 0:                                   # BigGAN.py:1121-1122
                    self.save(self.checkpoint_dir, self.counter)
                    if self._log_writer is not None:
                        self._log_writer.flush()
                if samples and (idx + 1) % self.print_freq == 0:                      # BigGAN.py:1125
                    self.save_samples(epoch, idx + 1)
                if self.swd_freq > 0 and self.counter % self.swd_freq == 0:
                    self._log_scores("SWD", self.swd())                                # (collective: every rank enters)
                if self.nn_freq > 0 and self.counter % self.nn_freq == 0:
                    self.save_neighbours(epoch, idx + 1)                               # (collective: every rank enters)
                if self.msssim_freq > 0 and self.counter % self.msssim_freq == 0:
                    self._log_scores("MS-SSIM", self.msssim())                         # (collective: every rank enters)
                if self.sv_freq > 0 and self.counter % self.sv_freq == 0 and self.rank == 0:
                    values, line, _ = self.singular_values()       # (rank 0 only: the weights are the same on every rank)
                    print(line, flush=True)
                    if self._log_writer is not None:
                        self._log_writer.add_scalars(self.counter - 1, values)
                if self.ps_freq > 0 and self.counter % self.ps_freq == 0:
                    self._log_scores("PS", self.power_spectrum())                      # (collective: every rank enters)
                if self.pr_freq > 0 and self.counter % self.pr_freq == 0:
                    self._log_scores("PRDC", self.prdc())                              # (collective: every rank enters)
            start_batch_id = 0                                                         # BigGAN.py:1164-1166
            self.save(self.checkpoint_dir, self.counter)
            if self._log_writer is not None:
                self._log_writer.flush()

    def save_recon_samples(self, epoch, idx):
        """--d_save_recon_samples (BigGAN.py:1050-1074): the targets and the reconstructions of the last D step as image
        grids ``<sample_dir>/BigGAN_{recon,txrecon}_{real,fake}_<epoch>_<idx>.png``."""
        from .utils import save_images, check_folder
        d = getattr(self, "_last_d_out", None)
        if not d:
            return []
        check_folder(self.sample_dir)
        grids = {}
        real = d["real_aug"].detach()
        if "coarse_upscaled" in d:
            grids["recon_fake"] = d["coarse_upscaled"]
            grids["recon_real"] = ops.avg_pooling(real) if self.d_reconstruction_halfres else real
        if "texture_upscaled" in d:
            tp = self.recon_plan["texture"]
            oy = min(max(int(d["rnd_offset_x"][0].item()), 0), tp["size"] - tp["feat_patch"]) * tp["f"]
            ox = min(max(int(d["rnd_offset_y"][0].item()), 0), tp["size"] - tp["feat_patch"]) * tp["f"]
            grids["txrecon_fake"] = d["texture_upscaled"]
            grids["txrecon_real"] = real[:, oy:oy + tp["patch"], ox:ox + tp["patch"], :]
        paths = []
        for name, img in grids.items():
            a = img.detach().float().cpu().numpy()
            dim = int(math.floor(math.sqrt(a.shape[0])))
            paths.append(save_images(a[:dim * dim], [dim, dim], os.path.join(
                self.sample_dir, "%s_%s_%02d_%05d.png" % (self.model_name, name, epoch, idx))))
        return paths

    # ---- sampling with the EMA weights (BigGAN.py:963-971) ------------------------------------
    def sample(self, z=None, cls_z=None, B=None, use_ema=True):
        """``self.fake_images``: generator(test_z, zero_cls_z, is_training=False, custom_getter=ema_getter).
        Trainables are read from their ExponentialMovingAverage shadows, non-trainables (``u``, moving
        statistics) from the live variables; batch norm uses the population statistics; the spectral-norm
        power iteration still advances ``u`` (its assign is a control dependency of w / sigma, ops.py:743)."""
        B = B or (z.shape[0] if z is not None else self.batch_size)
        self.sync_sharded_state()             # (data parallel with a sharded update: collective, every rank samples)
        if z is None:
            z = self.sample_z(B)
        if self.acgan and cls_z is None:
            cls_z = torch.zeros(B, self.n_labels, dtype=torch.float32, device=self.device)   # zero_cls_z
        arena = self.g_arena
        live = None
        if use_ema and arena.ema is not None:
            live = arena.params.clone()
            arena.params.copy_(arena.ema)
        try:
            S.set_default_store(self.store)
            ops.begin_run(None, 1)
            with torch.no_grad():
                img = self.generator(z, cls_z, is_training=False, reuse=True)
        finally:
            if live is not None:
                arena.params.copy_(live)
        return img

    # ---- in-training sample grids (BigGAN.py:980-1008, 1125-1230, 1397-1445) ---------------------
    def _generator_u(self):
        """The spectral-norm ``u`` vectors of the generator: the only state a no-grad, is_training=False generator pass
        writes (its power iteration advances them)."""
        return [self.store.vars[u] for w, u in self.store.sn_pairs.items() if w.startswith("generator/")]

    def _discriminator_u(self):
        """The spectral-norm ``u`` vectors of the discriminator (what its no-grad, is_training=False pass writes)."""
        return [self.store.vars[u] for w, u in self.store.sn_pairs.items() if w.startswith("discriminator/")]

    def generate(self, z, cls_z=None, ema=True, grid=None, gh=0, gw=0, _synced=False, with_discriminator=False,
                 _place=None, _consume=None):
        """BigGAN.py:1397-1445: images of a list of latents (and class vectors; None
        with --n_labels: zeros).  The list is padded to a multiple of ``batch_size`` by repeating entry 0 and runs
        ``batch_size`` at a time with is_training=False; ``ema`` reads the trainables from their moving averages,
        swapped in once for the whole call.  With ``grid`` (uint8 [gh*S, gw*S, c_dim] on the device) each batch goes straight
        into the byte grid at its tile offset (functional.image_tiles_u8) and the grid is returned: one batch of float
        images is live at a time.  Without it: the concatenated images, trimmed to len(z).

        Unlike ``sample()`` this leaves the model as it found it: the generator's ``u`` vectors are put back before
        every batch and after the last, so each image is a function of its latent alone and the training run does not
        depend on whether anybody looked at samples.  Under a sharded optimiser the caller runs
        ``sync_sharded_state()`` on every rank first (``_synced``); the generator passes themselves are local.

        ``with_discriminator``: every batch also runs ``discriminator(img, is_training=False, reuse=True)`` without the
        reconstruction heads, and the call returns ``(images or grid, {key: fp32 [n, ...]})`` with ``real`` [n,1] and,
        under --n_labels, ``cls`` [n,n_labels], trimmed to len(z).  The discriminator's ``u`` vectors are put back like
        the generator's.  (The reference builds this discriminator with is_training=True; under --bn_in_d the padding
        rows would then move the answer and the moving statistics, so this pass reads the population statistics.)
        ``_place`` (the sampling service): ``(table int32 [padded n, 4], arena uint8 [bytes])`` on the device - each
        batch goes through ``functional.image_place_u8`` with its rows of the table instead of being kept, and the arena
        takes the place of the images in the result.  ``_consume`` (the quality score): a callable that takes each batch of
        images, padding included, as it is produced; nothing is kept and the result is None."""
        import numpy as np

        def dev(a, width):
            if not torch.is_tensor(a):
                a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
            return a.to(device=self.device, dtype=torch.float32).reshape(-1, width)
        B = self.batch_size
        z = dev(z, self.z_dim)
        n = z.shape[0]
        if n == 0:
            raise ValueError("generate: no latents")
        if self.acgan:
            cls_z = (torch.zeros(n, self.n_labels, dtype=torch.float32, device=self.device) if cls_z is None
                     else dev(cls_z, self.n_labels))
            if cls_z.shape[0] != n:
                raise ValueError("generate: %d latents but %d class vectors" % (n, cls_z.shape[0]))
        else:
            cls_z = None
        pad = -n % B
        if pad:
            z = torch.cat([z, z[0:1].expand(pad, -1)])
            if cls_z is not None:
                cls_z = torch.cat([cls_z, cls_z[0:1].expand(pad, -1)])
        z = z.reshape(-1, 1, 1, self.z_dim)
        if not _synced:
            self.sync_sharded_state()
        self._wait_params("generator")
        arena = self.g_arena
        u_live = self._generator_u()
        sn_batches = list(getattr(self, "sn_batches", {}).get("generator", ()))
        if with_discriminator:
            self._wait_params("discriminator")
            u_live = u_live + self._discriminator_u()
            sn_batches += getattr(self, "sn_batches", {}).get("discriminator", ())
        if _place is not None and tuple(_place[0].shape) != (z.shape[0], 4):
            raise ValueError("generate: the placement table must be [%d,4], got %s" % (z.shape[0], tuple(_place[0].shape)))
        out, d_out = [], {}
        with torch.no_grad():
            u_saved = [u.clone() for u in u_live]
            live = None
            if ema and arena.ema is not None:
                live = arena.params.clone()
                arena.params.copy_(arena.ema)
            for sb in sn_batches:
                sb.local_only = True              # (a weight-sharded power iteration would be a collective)
            try:
                S.set_default_store(self.store)
                Fn.set_precision(self.precision)
                for b in range(0, z.shape[0], B):
                    if b and u_live:
                        torch._foreach_copy_(u_live, u_saved)
                    ops.begin_run(None, 1)
                    img = self.generator(z[b:b + B], None if cls_z is None else cls_z[b:b + B], is_training=False,
                                         reuse=True)
                    if with_discriminator:
                        for k, v in self.discriminator(img, is_training=False, reuse=True).items():
                            d_out.setdefault(k, []).append(v.float())
                    if _consume is not None:
                        _consume(img)
                    elif _place is not None:
                        Fn.image_place_u8(img, _place[0][b:b + B], _place[1])
                    elif grid is not None:
                        Fn.image_tiles_u8(img, grid, gh, gw, tile0=b)
                    else:
                        out.append(img)
            finally:
                for sb in sn_batches:
                    sb.local_only = False
                if u_live:
                    torch._foreach_copy_(u_live, u_saved)
                if live is not None:
                    arena.params.copy_(live)
        res = None if _consume is not None else (_place[1] if _place is not None else grid if grid is not None
                                                 else torch.cat(out)[:n])
        if with_discriminator:
            return res, {k: torch.cat(v)[:n] for k, v in d_out.items()}
        return res

    def static_sample_set(self):
        """(z [rounded_n,1,1,z_dim], class vectors [rounded_n,n_labels] or None) as fp32 numpy arrays: the static sample
        set of BigGAN.py:980-1002, drawn on first use (sampling.static_z / static_cls; --load_cls_samples_from replaces
        the class vectors, --save_cls_samples_to writes them)."""
        if self._static_set is None:
            import numpy as np
            from . import sampling as Sp
            _, rounded_n, _ = Sp.grid_plan(self.sample_num, self.batch_size)
            z = Sp.static_z(rounded_n, self.z_dim, self.static_sample_seed, self.z_trunc_sample).numpy()
            cls = None
            if self.acgan:
                cls = Sp.static_cls(self._label_table(), rounded_n, self.static_sample_seed)
                if self.args.load_cls_samples_from:
                    _, vectors = Sp.read_vectors(self.args.load_cls_samples_from, expect=rounded_n)
                    cls = np.asarray(vectors[:rounded_n], dtype=np.float32)
                    if cls.ndim != 2 or cls.shape[1] != self.n_labels:
                        raise ValueError("%s: class vectors of %s values, --n_labels is %d"
                                         % (self.args.load_cls_samples_from, cls.shape[1:], self.n_labels))
                if self.args.save_cls_samples_to and self.rank == 0:
                    Sp.write_vectors(self.args.save_cls_samples_to, cls)
            self._static_set = (z, cls)
        return self._static_set

    def _label_table(self):
        from . import sampling as Sp
        return self.labels if self.labels is not None else Sp.synthetic_label_table(self.n_labels)

    def save_samples(self, epoch, idx):
        """The sample grids of one ``print_freq`` event (BigGAN.py:1125-1230) into ``sample_dir``; returns their paths.
        ``<model>_ema_EE_IIIII.png`` / ``_noema_`` (--sample_ema), ``_morph_`` (--save_morphs: a bilinear blend of four
        static latents with an extrapolated border ring), ``_cls_EE_IIIII_TTT.png`` (--save_cls_samples with --n_labels:
        the static latents under class vectors that carry tag TTT).  With --static_sample_z the ema / noema grids show
        the static set, otherwise fresh latents from a generator of their own with zero class vectors.

        Every rank calls it (``sync_sharded_state`` is collective); rank 0 runs the generator and writes.  Nothing the
        training run reads is changed: parameters, moving averages, optimiser slots, statistics, every ``u``,
        ``self.gen`` and ``self.counter`` are bit-identical afterwards.  The grids are assembled as bytes on the device
        and cross to the host once, one byte per element; under BG_DEVICE_PNG=1 they are also encoded there (png.py) and
        only the files' bytes cross."""
        from . import png as Png, sampling as Sp
        from .utils import write_png, check_folder
        self.sync_sharded_state()
        if self.rank != 0:
            return []
        check_folder(self.sample_dir)
        B = self.batch_size
        dim, _, batches = Sp.grid_plan(self.sample_num, B)
        rng = Sp.event_rng(self.static_sample_seed, epoch, self.iterations_per_epoch, idx)
        paths = []

        def write(name, z, cls_z, ema, side):
            grid = torch.zeros(side * self.img_size, side * self.img_size, self.c_dim, dtype=torch.uint8,
                               device=self.device)
            self.generate(z, cls_z, ema=ema, grid=grid, gh=side, gw=side, _synced=True)
            path = os.path.join(self.sample_dir, name)
            if Png.enabled():                              # filtered and compressed where it lies (csrc/png.hip)
                with open(path, "wb") as f:
                    f.write(Png.encode_device(grid.reshape(-1), [(0,) + tuple(grid.shape)])[0])
                paths.append(path)
            else:
                paths.append(write_png(grid.cpu().numpy(), path))

        def plain(kind, ema):
            if self.static_sample_z:
                zs, cs = self.static_sample_set()
                z, cls_z = zs[:batches * B], (None if cs is None else cs[:batches * B])
            else:                                                                      # BigGAN.py:1004-1008
                z, cls_z = Sp.draw_z(batches * B, self.z_dim, self.sample_gen, self.z_trunc_sample), None
            write(Sp.sample_names(self.model_name, epoch, idx)[kind], z, cls_z, ema, dim)
        if self.generate_ema_samples:
            plain("ema", True)
        if self.generate_noema_samples:
            plain("noema", False)
        if self.save_morphs:                                                           # BigGAN.py:1169-1200
            zs, cs = self.static_sample_set()
            corners = Sp.morph_corners(self.sample_num, rng)
            z, cls_z = Sp.morph_latents([zs[i] for i in corners], None if cs is None else [cs[i] for i in corners], dim)
            write(Sp.sample_names(self.model_name, epoch, idx)["morph"], z, cls_z, True, dim + 2)
        if self.acgan and self.save_cls_samples:                                       # BigGAN.py:1202-1230
            zs, _ = self.static_sample_set()
            tag, cls_z = Sp.cls_grid_vectors(self._label_table(), self.n_labels, dim * dim, rng)
            write(Sp.sample_names(self.model_name, epoch, idx, tag)["cls"], zs[:dim * dim], cls_z, True, dim)
        return paths

    # ---- in-training monitors: quality, diversity, frequency check, precision / recall (metrics.py) ----
    def _dataset_files(self, root="./dataset"):
        """The dataset's file listing (None without a dataset folder), as the training loader would list it."""
        from . import data as D
        if not os.path.isdir(os.path.join(root, self.dataset_name)):
            return None
        files, _ = D.load_data(self.dataset_name, self.args.label_file, self.args.weight_file,
                               ignore_missing=self.args.ignore_missing_labels, n_labels=self.n_labels, root=root)
        return list(files)

    def monitor_plan(self, kind, root="./dataset"):
        """The plan of the monitor ``kind`` ("swd", "msssim", "ps" or "prdc") from its flags and the dataset's listing."""
        from .metrics import MONITORS
        plan_class, _, flags = MONITORS[kind]
        files = self._dataset_files(root)
        return plan_class(self.img_size, self.c_dim, self.batch_size, *[getattr(self, f) for f in flags],
                          self.static_sample_seed, n_files=None if files is None else len(files))

    def monitor_fake_inputs(self, plan):
        """(latents [n,1,1,z_dim], class vectors [n,n_labels] or None) of a monitor's fake set, n = ``plan.n_fake``: drawn
        from the plan's seeds, with --z_trunc_train's truncation and rows of the label table, the same at every event.
        (MS-SSIM: rows 2p and 2p + 1 are pair p - independent latents, one row of the label table for both.)"""
        z = plan.draw_latents(self.z_dim, self.z_trunc_train)
        return z, (plan.draw_labels(self._label_table()) if self.acgan else None)

    def monitor_real_batches(self, plan, root="./dataset"):
        """The real set of a monitor, at most ``batch_size`` images at a time on the device: with a dataset folder the
        first ``plan.n_stream`` files of the listing, or those that ``plan.real_order()`` names (MS-SSIM: a random matching
        of the first files, the pairs as consecutive rows), decoded and resized by the host path without flips (never
        taken from the training loader); without one, uniform noise from a generator of the metric's own."""
        B, M = self.batch_size, plan.n_stream
        if plan.from_files:
            import numpy as np
            from . import data as D
            image_data = D.ImageData(self.img_size, self.c_dim, True, False)
            files, order = self._dataset_files(root), plan.real_order()
            files = files[:M] if order is None else [files[i] for i in order]
            for lo in range(0, M, B):
                yield torch.from_numpy(np.stack([image_data.image_processing(f) for f in files[lo:lo + B]])).to(self.device)
        else:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(plan.seeds["real"])
            for lo in range(0, M, B):
                yield torch.rand(min(B, M - lo), self.img_size, self.img_size, self.c_dim, device=self.device,
                                 generator=gen) * 2.0 - 1.0

    def _monitor_event(self, kind, root="./dataset", details=False):
        """One event of the monitor ``kind`` (metrics.Monitor.event): its scores, or with ``details`` (scores, the runner,
        {tag: what ``finish`` returned}).  The runner is built at the kind's first event and kept with its real set; the
        fake set's inputs are drawn once, after the real set is measured.  Every rank calls it (``sync_sharded_state`` is
        collective); rank 0 computes, the others return {}."""
        from .metrics import MONITORS
        self.sync_sharded_state()
        if self.rank != 0:
            return ({}, None, {}) if details else {}
        with torch.no_grad():
            m = self._monitors.get(kind)
            if m is None:
                m = self._monitors[kind] = MONITORS[kind][1](self.monitor_plan(kind, root), self.device)

            def generate(ema, consume):
                if m.fake_inputs is None:
                    m.fake_inputs = self.monitor_fake_inputs(m.plan)
                self.generate(m.fake_inputs[0], m.fake_inputs[1], ema=ema, _synced=True, _consume=consume)

            out, sets = m.event(lambda: self.monitor_real_batches(m.plan, root), generate, self.generate_ema_samples,
                                self.generate_noema_samples, details)
        return (out, m, sets) if details else out

    def _log_scores(self, tag, scores):
        """Rank 0: the "TAG: name: value, ..." line of an event and, while a training log is open, its scalars.  Returns
        ``scores``."""
        if self.rank == 0:
            from .metrics import format_scores
            print(tag + ": " + format_scores(scores), flush=True)
            if getattr(self, "_log_writer", None) is not None:                       # (--phase test opens no log)
                self._log_writer.add_scalars(self.counter - 1, scores)
        return scores

    def _write_scores(self, path, scores):
        """Rank 0: one "name<TAB>value" row per score."""
        if self.rank == 0:
            with open(path, "w") as f:
                for k, v in scores.items():
                    f.write("%s\t%.6f\n" % (k, v))

    def swd(self, root="./dataset"):
        """The sliced Wasserstein scores of the current weights: {``swd_<side>``: 1e3 x distance per pyramid level,
        ``swd_avg``: their mean} for the moving averages and / or ``swd_noema_*`` for the live weights, as --sample_ema
        says.  The real set's descriptors are computed at the first call and kept; the fake set is regenerated through
        ``generate`` a batch at a time from latents drawn once.  Every rank calls it (``sync_sharded_state`` is
        collective); rank 0 computes, the others return {}.  Nothing the training run reads is changed."""
        return self._monitor_event("swd", root)

    def msssim(self, root="./dataset"):
        """The diversity score of the current weights: {``msssim``: the mean MS-SSIM of --msssim_pairs generated pairs} for
        the moving averages and / or ``msssim_noema`` for the live weights, as --sample_ema says; lower is more diverse,
        1.0 means that every pair is identical.  The first call adds ``msssim_real``, the same number over random pairs
        of dataset images (dataset-wide, not per class).  The pairs are regenerated through ``generate`` a batch at a
        time from latents and class vectors drawn once.  Every rank calls it (``sync_sharded_state`` is collective);
        rank 0 computes, the others return {}.  Nothing the training run reads is changed."""
        return self._monitor_event("msssim", root)

    # ---- singular-value monitor (spectrum.py) -----------------------------------------------------
    def singular_values(self):
        """The top --sv_k singular values of every ``/kernel`` variable of G and D, live weights: (scalars in the order
        they are logged, the "SV: ..." line, the event as ``spectrum.SingularValues.event`` returns it).  Runs on the
        current stream outside any captured graph; no collective, so only rank 0 needs to call it.  With --sn the
        scalars hold sv_sn_ratio_min / _max, the monitor's sigma_0 over the sigma that the last D or G run's spectral norm
        wrote.  Reads the weights; draws from the monitor's own generator only."""
        from . import spectrum
        self._wait_params()                    # (sharded update: the all-gather of the new parameters may be in flight)
        with torch.no_grad():
            if self._sv is None:
                self._sv = spectrum.SingularValues(self.store, self.device, self.sv_k, self.sv_iters, self.sv_tol)
            result = self._sv.event()
            sigma_of = None
            if self.sn:
                slots = {}
                for w in result["weights"]:
                    wn = getattr(self.store.vars[w["name"]], "bg_sn_wn", None)
                    if wn is not None and getattr(wn, "bg_sigma", None) is not None:
                        slots[w["name"]] = wn.bg_sigma
                if slots:
                    host = torch.cat([t.reshape(1) for t in slots.values()]).cpu().tolist()
                    table = dict(zip(slots.keys(), host))
                    sigma_of = table.get
        values, top = spectrum.scalars(result, self.sv_k, sigma_of)
        return values, spectrum.format_line(result, top), result

    def power_spectrum(self, root="./dataset", details=False):
        """The frequency check of the current weights: the radial power spectrum of --ps_images generated images against
        the real set's, as ``ps_dist`` (decades), ``ps_hf`` (above 0: excess fine structure, below 0: blur), ``ps_peak``
        and ``ps_peak_at`` (cycles per pixel) for the moving averages and / or the ``_noema`` forms for the live weights,
        as --sample_ema says.  The real set is measured at the first call; only its profile and 2-D sum are kept.  The
        fakes are regenerated through ``generate`` a batch at a time from latents and class vectors drawn once.  Every
        rank calls it (``sync_sharded_state`` is collective); rank 0 computes, the others return {}.  Nothing the
        training run reads is changed.  ``details``: return (scores, the runner, {tag: what ``finish`` returned})."""
        return self._monitor_event("ps", root, details)

    def save_power_spectrum(self, folder, root="./dataset"):
        """--phase test: ``ps.txt`` (one row per radius: r, r/S, n_r, L_real, L_fake (and L_fake_noema), D) and ``ps.png``
        (the mean 2-D spectra of the real and the fake set side by side, log10 over 8 decades) in ``folder``."""
        scores, m, sets = self.power_spectrum(root, details=True)
        return scores, ([] if self.rank != 0 else m.save(folder, m.real, sets))

    def prdc(self, root="./dataset", details=False):
        """Improved precision / recall and density / coverage of --pr_images generated images against the real set in the
        box-filtered pixel descriptors, as ``pr_precision``, ``pr_recall``, ``pr_density``, ``pr_coverage`` for the moving
        averages and / or the ``_noema`` forms for the live weights, as --sample_ema says.  The real descriptors and their
        radii are computed at the first call and kept.  The fakes are regenerated through ``generate`` a batch at a time
        from latents and class vectors drawn once; an event is the radii of the fake set, two cover passes and one
        reduction, and reads 32 bytes back.  Every rank calls it (``sync_sharded_state`` is collective); rank 0 computes,
        the others return {}.  Nothing the training run reads is changed.  ``details``: return (scores, the runner,
        {tag: what ``finish`` returned})."""
        return self._monitor_event("prdc", root, details)

    def save_prdc(self, folder, root="./dataset"):
        """--phase test: ``prdc.txt`` in ``folder``: one "name<TAB>value" row per score, then k, N, M and D."""
        scores, m, _ = self.prdc(root, details=True)
        if self.rank != 0:
            return scores, []
        path = os.path.join(folder, "prdc.txt")
        self._write_scores(path, scores)
        with open(path, "a") as f:
            for k, v in (("k", m.plan.k), ("N", m.plan.N), ("M", m.plan.M), ("D", m.plan.D)):
                f.write("%s\t%d\n" % (k, v))
        return scores, [path]

    # ---- nearest training images (neighbours.py) -------------------------------------------------
    def nn_plan(self, root="./dataset"):
        from .neighbours import NnPlan
        files = self._dataset_files(root)
        return NnPlan(self.img_size, self.c_dim, self.batch_size, self.nn_size, self.nn_images, self.static_sample_seed,
                      n_files=None if files is None else len(files))

    def nn_set_batches(self, plan, files):
        """The training set of the search, ``batch_size`` images at a time on the device, in listing order and unflipped:
        decoded by a thread pool, then resized and normalised on the device where the loader would do so
        (``data.device_input_enabled``), else by ``ImageData.image_processing``; the two are bit-identical.  The
        ``ImageData`` is the search's own: the training loader and its flip stream are never touched.  Without a dataset
        folder: ``neighbours.synthetic_batch``."""
        B = self.batch_size
        if not plan.from_files:
            from .neighbours import synthetic_batch
            for b in range((plan.N + B - 1) // B):
                yield synthetic_batch(plan, b, self.device)
            return
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from . import data as D
        image_data = D.ImageData(self.img_size, self.c_dim, True, False)
        on_device = D.device_input_enabled(self.device)
        with ThreadPoolExecutor(max_workers=8) as pool:
            for lo in range(0, plan.N, B):
                part = files[lo:min(lo + B, plan.N)]
                if on_device:
                    arrs = list(pool.map(lambda f: D.decode_file(image_data, f), part))
                    if all(D.packable(a, self.c_dim) for a in arrs):
                        yield D.PackedBatch(*D.pack_batch(arrs, [False] * len(arrs), self.img_size, self.c_dim,
                                                          pin=True)).to_device(self.device)
                        continue
                    imgs = list(pool.map(lambda a: D.finish_on_host(a, self.img_size, False), arrs))
                else:
                    imgs = list(pool.map(image_data.image_processing, part))
                yield torch.from_numpy(np.stack(imgs)).to(self.device)

    def _nn_set(self, root="./dataset"):
        """The resident training set (neighbours.NearestSet), built at the first call and kept."""
        if self._nn is None:
            from . import neighbours
            plan = self.nn_plan(root)
            files = self._dataset_files(root)
            s = neighbours.NearestSet(plan, self.device, files)
            for batch in self.nn_set_batches(plan, files):
                s.add(batch)
            self._nn = s.finish()
        return self._nn

    def _nn_fetch(self, index):
        """The full-size training image fp32 [S,S,C] (numpy) of a set index, by the host path; kept per index."""
        s = self._nn
        if index not in s.images:
            if s.plan.from_files:
                from . import data as D
                s.images[index] = D.ImageData(self.img_size, self.c_dim, True, False).image_processing(s.files[index])
            else:
                from .neighbours import synthetic_batch
                b, i = divmod(index, self.batch_size)
                s.images[index] = synthetic_batch(s.plan, b, self.device)[i].cpu().numpy()
        return s.images[index]

    def nearest(self, images=None, ema=True, k=None, root="./dataset", _samples=None):
        """The ``k`` (default --nn_k) nearest training images of ``images`` [Q,S,S,C] on the device, or else of the first
        min(sample_num, batch_size) images of the static sample set (``ema``: from the moving averages), in pixel space at
        the search side: {``dist`` [Q,k]: RMS difference per element in units of the [-1, 1] pixel scale, ``index``: rows of
        the listing, ``mirrored``: the hit is the mirror image (searched when --random_flip is true), ``files``}.  The
        training set's descriptors are computed at the first call and kept.  Every rank calls it (``sync_sharded_state`` is
        collective); rank 0 computes, the others return {}.  Nothing the training run reads is changed."""
        self.sync_sharded_state()
        if self.rank != 0:
            return {}
        with torch.no_grad():
            s = self._nn_set(root)
            if images is None:
                zs, cs = self.static_sample_set()
                n = min(self.sample_num, self.batch_size)
                images = self.generate(zs[:n], None if cs is None else cs[:n], ema=ema, _synced=True)
            if _samples is not None:
                _samples.append(images)
            return s.search(images, self.nn_k if k is None else k, bool(self.args.random_flip))

    def save_neighbours(self, epoch, idx, folder=None, names=None):
        """One --nn_freq event: for the moving averages and / or the live weights, as --sample_ema says, the grid
        ``<model>_nn_EE_IIIII.png`` (``_nn_noema_``) of the up to 8 samples closest to a training image, each followed by its
        neighbours, the table ``.txt`` beside it, the scalars ``nn_dist_min`` / ``nn_dist_mean`` and one "NN: ..." line.
        Collective like ``save_samples``; returns the paths written."""
        from . import neighbours
        from .utils import check_folder
        paths = []
        for prefix, ema, wanted in (("nn", True, self.generate_ema_samples), ("nn_noema", False, self.generate_noema_samples)):
            if not wanted:
                continue
            first = self._nn is None
            samples = []
            result = self.nearest(ema=ema, _samples=samples)                           # (collective: every rank enters)
            if self.rank != 0:
                continue
            folder_ = self.sample_dir if folder is None else folder
            check_folder(folder_)
            which = neighbours.event_names(self.model_name, epoch, idx, prefix) if names is None else names[prefix]
            paths += neighbours.write_event(result, samples[0].float().cpu().numpy(), self._nn_fetch, folder_, which)
            scalars = neighbours.scalars(result, prefix)
            if first:
                print("NN: set of " + self._nn.plan.describe(), flush=True)
            print("NN: " + ", ".join("%s: %.4f" % kv for kv in scalars.items()), flush=True)
            if getattr(self, "_log_writer", None) is not None:                       # (--phase test opens no log)
                self._log_writer.add_scalars(self.counter - 1, scalars)
        return paths

    def test(self):
        """--phase test (BigGAN.py:1372-1395): load the latest checkpoint and write ``test_num`` grids of
        floor(sqrt(min(sample_num, batch_size)))^2 EMA samples to ``<result_dir>/<model_dir>/``.  With --swd_freq > 0 the
        checkpoint's quality scores are printed and written to ``swd.txt`` beside them; with --nn_freq > 0 the nearest
        training images of its static samples go to ``nn.png`` / ``nn.txt`` (``nn_noema.*``); with --msssim_freq > 0 its
        diversity scores are printed and written to ``msssim.txt``; with --sv_freq > 0 ``sv.txt`` gets one row per monitored
        weight: name, rows, cols, the --sv_k singular values and their residuals; with --ps_freq > 0 the radial power
        spectra go to ``ps.txt`` and the mean 2-D spectra to ``ps.png``; with --pr_freq > 0 precision, recall, density and
        coverage go to ``prdc.txt``."""
        import numpy as np
        from .utils import save_images, check_folder
        could_load, _ = self.load(self.checkpoint_dir)
        result_dir = os.path.join(self.args.result_dir, self.model_dir)
        check_folder(result_dir)
        print(" [*] Load SUCCESS" if could_load else " [!] Load failed...")
        tot_num_samples = min(self.args.sample_num, self.batch_size)
        dim = int(np.floor(np.sqrt(tot_num_samples)))
        paths = []
        for i in range(self.args.test_num):
            samples = self.sample(B=self.batch_size).detach().cpu().numpy()
            paths.append(save_images(samples[:dim * dim, :, :, :], [dim, dim],
                                     result_dir + '/' + self.model_name + '_test_{}.png'.format(i)))
        if self.swd_freq > 0:
            self._write_scores(os.path.join(result_dir, "swd.txt"), self._log_scores("SWD", self.swd()))
        if self.nn_freq > 0:
            paths += self.save_neighbours(0, 0, folder=result_dir,
                                          names={p: {"png": p + ".png", "txt": p + ".txt"} for p in ("nn", "nn_noema")})
        if self.msssim_freq > 0:
            self._write_scores(os.path.join(result_dir, "msssim.txt"), self._log_scores("MS-SSIM", self.msssim()))
        if self.ps_freq > 0:
            scores, written = self.save_power_spectrum(result_dir)
            self._log_scores("PS", scores)
            paths += [p for p in written if p.endswith(".png")]
        if self.pr_freq > 0:
            self._log_scores("PRDC", self.save_prdc(result_dir)[0])
        if self.sv_freq > 0 and self.rank == 0:
            _, line, result = self.singular_values()
            print(line, flush=True)
            with open(os.path.join(result_dir, "sv.txt"), "w") as f:
                for w in result["weights"]:
                    f.write("\t".join([w["name"], str(w["rows"]), str(w["cols"])] + ["%.9g" % x for x in w["sv"]]
                                      + ["%.3g" % x for x in w["resid"]]) + "\n")
        return paths

    # ---- --phase service (BigGAN.py:1298-1369) -----------------------------------------------
    def _serve_group(self, group):
        """Run one group of a round (service.Group) on the device -> (arena uint8 [arena_bytes], {key: fp32 [total, ...]})
        as numpy arrays on the host.  The latents go up once, ``generate`` swaps the moving averages in once and runs
        the generator, optionally the discriminator, and one placement launch per batch; the strips come back in one
        copy into a pinned buffer, the discriminator's outputs, stacked column-wise, in another.  Under BG_DEVICE_PNG=1
        the strips are encoded in the arena (png.encode_device) and the first result is {request path: PNG bytes}."""
        from . import png as Png
        dev = self.device
        arena = torch.zeros(group.arena_bytes, dtype=torch.uint8, device=dev)
        table = torch.from_numpy(group.table).to(dev)
        z = torch.from_numpy(group.z).to(dev)
        cls_z = None if group.cls is None else torch.from_numpy(group.cls).to(dev)
        res = self.generate(z, cls_z, ema=group.ema, with_discriminator=group.use_discriminator, _place=(table, arena))
        device_png = Png.enabled()
        if not device_png:
            host = torch.empty(group.arena_bytes, dtype=torch.uint8, pin_memory=True)
            host.copy_(arena, non_blocking=True)
        outs = {}
        if group.use_discriminator:
            keys = sorted(res[1])
            stacked = torch.cat([res[1][k].reshape(group.total, -1) for k in keys], dim=1).cpu()    # (synchronises)
            col = 0
            for k in keys:
                w = res[1][k].numel() // group.total
                outs[k] = stacked[:, col:col + w].numpy()
                col += w
        if device_png:                                     # every strip of the group in one launch of each kernel
            served = [r for r in group.files if r.n]
            S_, C_ = self.img_size, self.c_dim
            files = Png.encode_device(arena, [(r.offset, S_, r.n * S_, C_) for r in served])
            return {r.path: f for r, f in zip(served, files)}, outs
        torch.cuda.current_stream().synchronize()
        return host.numpy(), outs

    def _serve_round(self, rnd, request_dir, pool):
        """Answer a planned round (service.Round); returns when every response is written.  Responses are encoded by
        ``pool`` while the next group runs (zlib releases the GIL).  Returns the number of files answered with images."""
        from . import service as Sv
        pending = [pool.submit(Sv.write_error, path, msg) for path, msg in rnd.errors]
        served = 0
        for group in rnd.groups:
            try:
                if group.load_checkpoint is not None:
                    self.load_checkpoint(group.load_checkpoint)
                arena, outs = self._serve_group(group) if group.total else (None, {})
            except (OSError, KeyError, ValueError) as e:       # (a checkpoint that is not there or does not fit)
                if group.load_checkpoint is None:
                    raise
                pending += [pool.submit(Sv.write_error, req.path, "load_checkpoint %s: %s" % (group.load_checkpoint, e))
                            for req in group.files]
                continue
            for req in group.files:
                pending.append(pool.submit(Sv.write_response, req, request_dir, arena, outs, self.img_size, self.c_dim))
                served += 1 if req.n else 0
        for f in pending:
            f.result()
        return served

    def service(self, poll_s=0.005, idle_timeout_s=None):
        """--phase service (BigGAN.py:1298-1369): load the latest checkpoint, then answer the request files of
        ``--request_dir`` until one of them says ``quit``.  ``NAME.txt`` holds latents (utils.read_vectors) and is
        answered with ``NAME.png``, the strip of its images, and under ``use_discriminator=1`` with ``NAME_<key>.out``
        (utils.write_vectors).  The pending files of a poll round share generator batches (service.plan_round).
        ``idle_timeout_s``: return after this long without a request (None: never).  Returns the number of files answered
        with images."""
        from concurrent.futures import ThreadPoolExecutor
        from . import service as Sv
        from .utils import check_folder
        if self.world > 1:
            raise RuntimeError("--phase service runs in one process (world size %d)" % self.world)
        could_load, _ = self.load(self.checkpoint_dir)
        print(" [*] Load SUCCESS" if could_load else " [!] Load failed...")
        request_dir = check_folder(self.args.request_dir)
        served, last = 0, time.monotonic()
        with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
            while True:
                paths = Sv.list_requests(request_dir)
                if paths:
                    rnd = Sv.plan_round(Sv.read_requests(paths), self.batch_size, self.z_dim, self.n_labels if self.acgan
                                        else 0, self.img_size, self.c_dim)
                    served += self._serve_round(rnd, request_dir, pool)
                    if rnd.quit is not None:
                        os.remove(rnd.quit)                                            # BigGAN.py:1324-1326
                        return served
                    last = time.monotonic()
                elif idle_timeout_s is not None and time.monotonic() - last >= idle_timeout_s:
                    return served
                time.sleep(poll_s)

    # ---- checkpoints (BigGAN.py:1255-1284) ---------------------------------------------------
    def _ckpt_dir(self, checkpoint_dir):
        return os.path.join(checkpoint_dir, self.model_dir)

    def state_tensors(self):
        """name -> tensor, keyed like a TF checkpoint of the reference graph: variables by their scope
        names, ``<var>/ExponentialMovingAverage`` shadows, Adam slots ``<var>/Adam`` (m) and ``<var>/Adam_1`` (v).

        Key convention (differs from the reference's swapping_saver, BigGAN.py:1018): here ``<var>`` is the LIVE
        weight and ``<var>/ExponentialMovingAverage`` its shadow, as in a plain tf.train.Saver.  The reference's
        swapping saver stores them the other way round (averages under the variable names), so a converter between
        the two formats must swap the pair for every generator trainable."""
        out = {}
        for k, v in self.store.vars.items():
            out[k] = v.detach()
        for group, arena in self.store.arenas.items():
            for name in arena.names:
                out[name + "/Adam"] = arena.view(arena.m, name)
                out[name + "/Adam_1"] = arena.view(arena.v, name)
                if arena.ema is not None:
                    out[name + "/ExponentialMovingAverage"] = arena.view(arena.ema, name)
        return out

    def save(self, checkpoint_dir, step):
        """``<checkpoint_dir>/<model_dir>/BigGAN.model-<step>.safetensors`` + a TF-style ``checkpoint`` index.
        Under data parallelism every rank calls it (the sharded optimiser state is gathered first); rank 0 writes."""
        from safetensors.torch import save_file
        self.sync_sharded_state()
        if self.rank != 0:
            return None
        d = self._ckpt_dir(checkpoint_dir)
        os.makedirs(d, exist_ok=True)
        tensors = {k: v.detach().to("cpu").contiguous().clone() for k, v in self.state_tensors().items()}
        tensors["_meta/steps"] = torch.tensor([self.counter, self.d_arena.step, self.g_arena.step], dtype=torch.int64)
        name = "%s.model-%d" % (self.model_name, int(step))
        save_file(tensors, os.path.join(d, name + ".safetensors"))
        with open(os.path.join(d, "checkpoint"), "w") as f:
            f.write('model_checkpoint_path: "%s"\n' % name)
        self._prune_checkpoints(d)
        return os.path.join(d, name + ".safetensors")

    def _prune_checkpoints(self, d):
        """swapping_saver(max_to_keep=keep_checkpoints) (BigGAN.py:1018): keep the newest N checkpoint files."""
        keep = int(getattr(self.args, "keep_checkpoints", 0) or 0)
        if keep <= 0:
            return
        pre, suf = self.model_name + ".model-", ".safetensors"
        found = []
        for f in os.listdir(d):
            if f.startswith(pre) and f.endswith(suf):
                try:
                    found.append((int(f[len(pre):-len(suf)]), f))
                except ValueError:
                    pass
        for _, f in sorted(found)[:-keep]:
            os.remove(os.path.join(d, f))

    def load_checkpoint(self, checkpoint_path):
        from safetensors.torch import load_file
        if not checkpoint_path.endswith(".safetensors"):
            checkpoint_path += ".safetensors"
        tensors = load_file(checkpoint_path)
        dst = self.state_tensors()
        missing = [k for k in dst if k not in tensors]
        if missing:
            raise KeyError("checkpoint %s lacks %d tensors, e.g. %s" % (checkpoint_path, len(missing), missing[:3]))
        with torch.no_grad():
            for k, t in dst.items():
                src = tensors[k]
                if tuple(src.shape) != tuple(t.shape):
                    raise ValueError("checkpoint tensor %s has shape %s, model expects %s"
                                     % (k, tuple(src.shape), tuple(t.shape)))
                t.copy_(src.to(t.device))
        steps = tensors.get("_meta/steps")
        ckpt_name = os.path.basename(checkpoint_path)[:-len(".safetensors")]
        counter = int(ckpt_name.split('-')[-1])
        if steps is not None:
            self.d_arena.step, self.g_arena.step = int(steps[1]), int(steps[2])
        self.counter = counter
        print(" [*] Successfully read {}".format(ckpt_name))
        return True, counter

    def load(self, checkpoint_dir):
        print(" [*] Reading checkpoints...")
        d = self._ckpt_dir(checkpoint_dir)
        if getattr(self.args, "checkpoint", ""):
            return self.load_checkpoint(self.args.checkpoint)
        index = os.path.join(d, "checkpoint")
        if os.path.exists(index):
            line = open(index).read().strip().splitlines()[0]
            name = line.split(":", 1)[1].strip().strip('"')
            return self.load_checkpoint(os.path.join(d, name))
        print(" [*] Failed to find a checkpoint")
        return False, 0

    @property
    def model_dir(self):
        """BigGAN.py:1246-1253."""
        sn = '_sn' if self.sn else ''
        return "{}_{}_{}_{}_{}{}".format(self.model_name, self.dataset_name, self.gan_type, self.img_size,
                                         self.z_dim, sn)
