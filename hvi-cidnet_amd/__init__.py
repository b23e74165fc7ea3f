"""hvi-cidnet_amd: MI355X-native CIDNet forward/backward hot path.

Hand-written gfx950 HIP kernels behind a C ABI (include/cidnet_hip.h, csrc/), wrapped as
torch.autograd.Function ops (ops.py) and assembled into modules whose names, constructor arguments,
attributes and state_dict keys equal the reference's net/CIDNet.py (cidnet.py, lca.py,
transformer_utils.py, hvi_transform.py).  There is no CPU or ATen fallback: tensors must live on a
ROCm device and libcidnet_hip.so must be built (`python hvi-cidnet_amd/build.py`).
"""
from . import _lib  # noqa: F401
from .cidnet import CIDNet
from .cidnet_mssa import CIDNet as CIDNet_MSSA, SpatialAttention
from .cidnet_tnsm import CIDNet_TNSM
from .tnsm import HV_TNSM, I_TNSM, TrainableNoiseSuppression
from .hvi_transform import RGB_HVI
from .lca import CAB, IEL, HV_LCA, I_LCA
from .transformer_utils import LayerNorm, NormDownsample, NormUpsample
from .losses import L1Loss, SSIM, EdgeLoss, CIDNetLoss, PerceptualLoss, LPIPSLoss, FFTLoss, VGGFeatureExtractor, tnsm_noise_loss
from .inference import enhance, load_weights, save_pretrained, pad_to_multiple
from .schedule import WarmupCosineLR
from . import metrics
from .metrics import evaluate, folder_pairs, nested_folder_pairs, group_means, evaluate_unpaired, folder_images, NiqeParams, load_niqe_params, loe, loe_counts, loe_grid, jpeg_quant_plan, jpeg_roundtrip_u8, LpipsParams, load_lpips_params, lpips, lpips_layers, lpips_features, lpips_feature_sizes, gt_mean_scale, ciede2000, ciede2000_map, ciede2000_lab, ciede2000_tables, BrisqueParams, load_brisque_params, brisque, brisque_features, brisque_score, brisque_gray, brisque_half, brisque_mscn, brisque_fit, brisque_plan
from . import data
from .data import ResidentPairs, TrainBatches, epoch_plan, scene_epoch_plan, scene_pairs, crop_flip, arena_layout, gamma_table
from . import image_io
from .image_io import ingest, egress, enhance_u8, enhance_folder, EnhanceReport, tile_plan, TilePlan, ingest_tiles, egress_tiles, png_plan, PngPlan, png_zlib_u8, png_file, png_encode_u8, jpeg_encode_plan, JpegEncodePlan, jpeg_scan_u8, jpeg_file, jpeg_encode_u8
from .dp import StepLog, TensorLog, tensor_stats_plan
from .fit import fit, run_epoch, epoch_stats, diagnose_epoch, write_preview
from .ops import set_storage_dtype, set_precision, set_math_levels

__all__ = ["CIDNet", "CIDNet_MSSA", "SpatialAttention", "CIDNet_TNSM", "HV_TNSM", "I_TNSM", "TrainableNoiseSuppression", "RGB_HVI", "CAB", "IEL", "HV_LCA", "I_LCA", "LayerNorm", "NormDownsample", "NormUpsample", "L1Loss", "SSIM", "EdgeLoss", "CIDNetLoss", "tnsm_noise_loss", "PerceptualLoss", "LPIPSLoss", "FFTLoss", "VGGFeatureExtractor", "enhance", "load_weights", "save_pretrained", "pad_to_multiple",
           "WarmupCosineLR", "set_storage_dtype", "set_precision", "set_math_levels", "metrics", "evaluate", "folder_pairs", "nested_folder_pairs", "group_means", "evaluate_unpaired", "folder_images", "NiqeParams",
           "load_niqe_params", "loe", "loe_counts", "loe_grid", "jpeg_quant_plan", "jpeg_roundtrip_u8", "LpipsParams", "load_lpips_params", "lpips", "lpips_layers", "lpips_features", "lpips_feature_sizes", "gt_mean_scale", "ciede2000", "ciede2000_map", "ciede2000_lab", "ciede2000_tables", "BrisqueParams", "load_brisque_params", "brisque", "brisque_features", "brisque_score", "brisque_gray", "brisque_half", "brisque_mscn", "brisque_fit", "brisque_plan", "data", "ResidentPairs", "TrainBatches", "epoch_plan", "scene_epoch_plan", "scene_pairs", "crop_flip", "arena_layout", "gamma_table",
           "fit", "run_epoch", "epoch_stats", "StepLog", "TensorLog", "tensor_stats_plan", "diagnose_epoch", "write_preview", "image_io", "ingest", "egress", "enhance_u8", "enhance_folder", "EnhanceReport", "tile_plan", "TilePlan", "png_plan", "PngPlan", "png_zlib_u8", "png_file", "png_encode_u8", "jpeg_encode_plan", "JpegEncodePlan", "jpeg_scan_u8", "jpeg_file", "jpeg_encode_u8",
           "ingest_tiles", "egress_tiles"]
