"""treedetection_amd — MI355X-native drop-in for the prediction stage of Jonetz/TreeDetection.

Public surface mirrors the reference package (TreeDetection/__init__.py:3-9): process_files, preprocess_files,
predict_tiles, postprocess_files, predict_on_model, Predictor, get_config, setup_model_cfg, clean_crowns; evaluate / evaluate_dirs restate
its supplementary/evaluation_compute_scores.py. The model forward runs in
libtreedet_hip.so (hand-written HIP for gfx950) behind the C ABI of include/treedet.h; there is no CPU fallback.
"""
__version__ = "0.1.0"

from .cleaning import (candidate_pairs, candidate_pairs_host, clean_crowns, clean_crowns_file,  # noqa: F401
                       ring_pairs_iou)
from .config import Config, get_config, setup_model_cfg  # noqa: F401
from .detection import (cleanup_files, postprocess_files, predict_on_model, predict_tiles,  # noqa: F401
                        preprocess_files, process_files)
from .engine import Engine  # noqa: F401
from .evaluation import (box_pairs_ab, clip_predictions, crown_iou_matrix, evaluate, evaluate_dirs,  # noqa: F401
                         load_annotations, load_predictions, match_crowns)
from .prediction import Predictor  # noqa: F401
from .treetops import (crown_treetops, find_treetops, gaussian_weights, smooth_height, treetop_marks,  # noqa: F401
                       treetops_file)
