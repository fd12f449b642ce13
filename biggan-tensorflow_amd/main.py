"""Command-line surface of the reference (``/root/reference/main.py:9-147``): the same 119 flags
with the same names, types and defaults, table-driven.  Flags whose features are outside the
MI355X hot path are accepted here and rejected when the model is built (``model.BigGAN.__init__``).

    python -m biggan_tensorflow_amd.main --phase train --gan_type hinge --img_size 128 --ch 64 --batch_size 64
"""
import argparse

from .utils import check_folder, str2bool

B, I, F, T = str2bool, int, float, str

# (name, type, default)  -- order follows main.py:9-147
FLAGS = [
    ("phase", T, "train"), ("dataset", T, "celebA-HQ"),
    ("epoch", I, 50), ("iteration", I, 10000), ("batch_size", I, 16), ("virtual_batches", I, 1),
    ("ch", I, 64), ("d_ch", I, 0), ("deep", B, False),
    ("print_freq", I, 250), ("save_freq", I, 1000), ("histogram_freq", I, 125), ("keep_checkpoints", I, 5),
    ("g_lr", F, 0.00005), ("d_lr", F, 0.0002),
    ("beta1", F, 0.0), ("beta2", F, 0.9), ("moving_decay", F, 0.999),
    ("z_dim", I, 256), ("shared_z", I, 0), ("c_dim", I, 3), ("alpha_mask", B, True), ("g_alpha_helper", B, True),
    ("first_split_ratio", I, 3), ("z_reconstruct", B, False), ("sn", B, True), ("bn_in_d", B, False),
    ("bias_in_d", B, False), ("bias_in_sa", B, True), ("bn_type", T, "batch_norm"), ("bn_momentum", F, 0.98),
    ("bn_renorm_rmax", F, 1.5), ("bn_renorm_dmax", F, 0.5), ("bn_renorm_momentum", F, 0.9),
    ("bn_renorm_shared", B, False), ("g_regularization", T, "ortho_cosine"), ("g_regularization_factor", F, 0.0001),
    ("conv_padding", T, "reflect"), ("upsampling_method", T, "deconv4"), ("downsampling_method", T, "strided_conv3"),
    ("g_conv", T, "deconv3"), ("g_grow_factor", F, 2.0), ("d_grow_factor", F, 2.0),
    ("g_sa_size", I, 0), ("d_sa_size", I, 0), ("sa_size", I, 0),
    ("gan_type", T, "ra-dragan"), ("d_loss_func", T, ""), ("activation", T, "prelu"), ("ld", F, 10.0),
    ("multi_head", B, False), ("d_flood", F, 0.1), ("g_flood", F, 0.05),
    ("n_critic", I, 1),
    ("img_size", I, 256), ("sample_num", I, 64), ("static_sample_z", B, True), ("static_sample_seed", I, 123456789),
    ("z_trunc_train", B, True), ("z_trunc_sample", B, True), ("save_morphs", B, False), ("sample_ema", T, "ema"),
    ("random_flip", B, True), ("da_policy", T, "full"),
    ("n_labels", I, 0), ("cls_embedding", B, False), ("cls_embedding_size", I, 0), ("cls_embedding_concat", B, False),
    ("label_file", T, ""), ("ignore_missing_labels", B, False), ("cls_loss_type", T, "logistic"),
    ("weight_file", T, ""), ("g_first_level_dense_layer", B, True), ("g_other_level_dense_layer", B, False),
    ("g_no_last_resblock", B, False), ("g_z_dense_concat", B, False), ("d_cls_dense_layers", B, False),
    ("d_compat_use_sn_in_classification", B, False), ("d_compat_use_sn_in_critic_output", B, True),
    ("g_mixed_resblocks", B, False), ("g_mixed_resblock_ch_div", F, 2.0), ("g_final_layer", B, False),
    ("g_final_layer_extra", B, False), ("g_final_layer_extra_bias", B, False), ("g_final_kernel", T, "3"),
    ("g_final_kernel_extra", T, "3"), ("g_final_layer_shortcuts", B, False), ("g_final_layer_shortcuts_after", I, 0),
    ("g_final_mixed_conv", B, False), ("g_final_mixed_conv_stacks", I, 2), ("g_final_mixed_conv_z_layers", T, "none"),
    ("g_final_mixed_nodeconv2", B, False), ("g_rgb_mix_kernel", I, 3), ("d_cls_loss_weight", F, 5.0),
    ("g_cls_loss_weight", F, 1.0), ("save_cls_samples", B, False), ("cls_loss_weights", T, ""),
    ("save_cls_samples_to", T, ""), ("load_cls_samples_from", T, ""), ("d_reconstruction", B, False),
    ("d_reconstruction_halfres", B, False), ("d_reconstruction_texture", B, False), ("d_tex_recon_feat_size", I, 16),
    ("d_tex_recon_patch_div", I, 4), ("d_recon_ch", I, 64), ("d_tex_recon_ch", I, 96), ("d_recon_ld", F, 1.0),
    ("d_tex_recon_ld", F, 0.5), ("d_recon_bn_after_act", B, False), ("d_save_recon_samples", B, False),
    ("d_final_conv", B, False),
    ("test_num", I, 10), ("allow_growth", B, False),
    ("checkpoint", T, ""), ("checkpoint_dir", T, "checkpoint"), ("result_dir", T, "results"), ("log_dir", T, "logs"),
    ("sample_dir", T, "samples"), ("request_dir", T, "request"),
]


# Extensions of this build (not flags of the reference, kept out of FLAGS):
#   --precision fp32        the reference's arithmetic (ops.py:14): fp32 tensors, fp32 MFMA          [default]
#               bf16-staged fp32 tensors, conv / large GEMM operands rounded to bf16 while staged, fp32 accumulate
#               bf16        BASELINE configs 3-5: bf16-resident activations + packed bf16 weights, fp32 accumulate,
#                           fp32 master weights / optimiser / statistics
#   the default can also be given by the environment variable BIGGAN_PRECISION
#   --swd_freq N            every N iterations: the sliced Wasserstein scores of the generator (metrics.py) as scalars in
#                           the event file and one "SWD: ..." line; 0 (default) is off.  --phase test: computed once
#   --swd_images M          images per set, rounded down to a power of two (and to the number of dataset files)
#   --nn_freq N             every N iterations: the nearest training images of the static samples in pixel space
#                           (neighbours.py): a grid and a table next to the sample grids, scalars nn_dist_min / nn_dist_mean
#                           and one "NN: ..." line; 0 (default) is off.  --phase test: computed once
#   --nn_k K                neighbours per sample, 1..8
#   --nn_size S             side of the search descriptors, a power of two >= 8; min(img_size, S) is used
#   --nn_images M           the first M files of the listing; 0 (default): all of them (capped by BG_NN_GB, default 8 GiB)
#   --msssim_freq N         every N iterations: the diversity score of the generator, the mean MS-SSIM of generated pairs that
#                           share a class vector (metrics.py; lower is more diverse, 1.0 is collapse), as scalars msssim /
#                           msssim_noema in the event file and one "MS-SSIM: ..." line; the first event adds msssim_real,
#                           the same over random pairs of dataset images (dataset-wide, not per class); 0 (default) is
#                           off.  --phase test: computed once
#   --msssim_pairs P        generated pairs per event
#   --sv_freq N             every N iterations: the top singular values of every weight matrix of G and D (spectrum.py,
#                           csrc/spectrum.hip) as scalars sv/<variable>/s0 .. in the event file with sv_g_max, sv_d_max,
#                           sv_resid_max (and sv_sn_ratio_min / _max with --sn) and one "SV: ..." line; 0 (default) is
#                           off.  --phase test: computed once, written to sv.txt
#   --sv_k K                values per weight, 1..4
#   --sv_iters T            iterations per round of the block power iteration (at most 8 rounds per event)
#   --sv_tol R              rounds stop once every reported residual is <= R: some true sigma^2 then lies within
#                           R sigma_0^2 of each reported value squared
#   --ps_freq N             every N iterations: the radial power spectrum of --ps_images generated images against the real
#                           set's (metrics.py, csrc/powerspec.hip): scalars ps_dist (decades between the log profiles),
#                           ps_hf (above 0: excess fine structure, below 0: blur), ps_peak / ps_peak_at (height and
#                           frequency in cycles per pixel of the largest spike: what a transposed or sub-pixel
#                           up-convolution leaves at the Nyquist frequencies) in the event file and one "PS: ..." line,
#                           the _noema forms as --sample_ema says; 0 (default) is off.  --phase test: computed once,
#                           ps.txt (one row per radius) and ps.png (the mean 2-D spectra, real beside fake) are written
#   --ps_images M           generated (and real) images per event
#   --pr_freq N             every N iterations: improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage
#                           (Naeem et al. 2020) of --pr_images generated images against as many real ones, in the
#                           box-filtered pixel descriptors of the memorisation check (metrics.py, csrc/prdc.hip): scalars
#                           pr_precision, pr_density (samples off the data manifold lower them) and pr_recall, pr_coverage
#                           (dropped modes lower them) in the event file and one "PRDC: ..." line, the _noema forms as
#                           --sample_ema says; 0 (default) is off.  --phase test: computed once, prdc.txt is written
#   --pr_images M           generated images per event, and real ones (at most the number of dataset files); > --pr_k
#   --pr_k K                the neighbour whose distance is a row's radius, 1..8
#   --pr_size S             side of the descriptors, a power of two >= 8; min(img_size, S) is used
EXTRA_FLAGS = [("precision", T, None), ("swd_freq", I, 0), ("swd_images", I, 2048),
               ("nn_freq", I, 0), ("nn_k", I, 3), ("nn_size", I, 64), ("nn_images", I, 0),
               ("msssim_freq", I, 0), ("msssim_pairs", I, 1024),
               ("sv_freq", I, 0), ("sv_k", I, 3), ("sv_iters", I, 8), ("sv_tol", F, 1e-2),
               ("ps_freq", I, 0), ("ps_images", I, 1024),
               ("pr_freq", I, 0), ("pr_images", I, 4096), ("pr_k", I, 3), ("pr_size", I, 64)]


def build_parser():
    parser = argparse.ArgumentParser(description="MI355X-native BigGAN training step (flag surface of the reference)")
    for name, typ, default in FLAGS + EXTRA_FLAGS:
        parser.add_argument("--" + name, type=typ, default=default)
    return parser


def check_args(args, make_dirs=True):
    """main.py:152-176: creates the four output folders; the two sanity checks only print."""
    if make_dirs:
        for d in (args.checkpoint_dir, args.result_dir, args.log_dir, args.sample_dir):
            check_folder(d)
    if not args.epoch >= 1:
        print('number of epochs must be larger than or equal to one')
    if not args.batch_size >= 1:
        print('batch size must be larger than or equal to one')
    return args


def parse_args(argv=None, make_dirs=True):
    import os
    args = build_parser().parse_args(argv)
    if args.precision is None:
        args.precision = os.environ.get("BIGGAN_PRECISION", "fp32")
    return check_args(args, make_dirs)


def main(argv=None):
    args = parse_args(argv)
    if args is None:
        exit()
    import torch
    from . import parallel
    from .model import BigGAN
    rank, world, local = parallel.init_from_env()        # torchrun: one process per GPU, RCCL
    if torch.cuda.is_available():
        torch.cuda.set_device(local % torch.cuda.device_count())
    gan = BigGAN(args)
    gan.build_model()
    if args.phase == 'train':
        gan.log_events = True                             # loss scalars and variable histograms into <log_dir>/<model_dir>/
        gan.train(samples=True)                           # sample grids every --print_freq iterations (BigGAN.py:1125)
        print(" [*] Training finished!")
    elif args.phase == 'test':
        gan.test()
        print(" [*] Test finished!")
    elif args.phase == 'service':
        gan.service()                                     # answers the latent files of --request_dir until one says quit
        print(" [*] Service finished!")
    else:
        raise NotImplementedError("--phase %s: the phases are train, test and service" % args.phase)


if __name__ == '__main__':
    main()
