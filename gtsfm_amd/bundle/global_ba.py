"""Global bundle adjustment, the last stage of the reference pipeline (gtsfm/bundle/global_ba.py): the class the
reference's configurations name; all behaviour is BundleAdjustmentOptimizer's."""
from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer


class GlobalBundleAdjustment(BundleAdjustmentOptimizer):
    """Bundle adjustment over every camera and landmark of the scene."""
