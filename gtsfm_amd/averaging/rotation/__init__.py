from gtsfm_amd.averaging.rotation.rotation_averaging_base import RotationAveragingBase  # noqa: F401
from gtsfm_amd.averaging.rotation.shonan import ShonanRotationAveraging  # noqa: F401
