"""Dense multi-view stereo: view selection, PatchmatchNet depth maps, fusion, voxel downsampling."""
from gtsfm_amd.densify.mvs_patchmatchnet import MVSPatchmatchNet  # noqa: F401
from gtsfm_amd.densify.patchmatchnet import PatchmatchNetDepthEstimator, pack_patchmatchnet_weights  # noqa: F401
