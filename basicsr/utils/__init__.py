from .color_util import rgb2ycbcr_pt
from .diffjpeg import DiffJPEG, quality_to_factor
from .img_process_util import USMSharp, filter2D, usm_sharp
from .knn_probe import FeatureTaps, classification_report, knn_probe, select_hook_modules, train_test_indices
from .logger import get_env_info, get_root_logger
from .matlab_functions import imresize
from .misc import get_time_str, make_exp_dirs, mkdir_and_rename, scandir, set_random_seed
from .mosaic_util import dm, dm_matlab, masks_CFA_Bayer, mosaic_CFA_Bayer
from .tsne import neighbour_label_share, pca_init_from_sqdist, tsne_embed

__all__ = ["get_root_logger", "get_env_info", "set_random_seed", "get_time_str", "mkdir_and_rename", "make_exp_dirs",
           "scandir", "DiffJPEG", "quality_to_factor", "imresize", "masks_CFA_Bayer", "mosaic_CFA_Bayer", "dm", "dm_matlab",
           "filter2D", "usm_sharp", "USMSharp", "FeatureTaps", "classification_report", "knn_probe", "select_hook_modules",
           "train_test_indices", "tsne_embed", "pca_init_from_sqdist", "neighbour_label_share", "rgb2ycbcr_pt"]
