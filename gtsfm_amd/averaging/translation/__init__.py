"""Translation averaging (gtsfm/averaging/translation)."""
from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationAveraging1DSFM
from gtsfm_amd.averaging.translation.translation_averaging_base import TranslationAveragingBase

__all__ = ["TranslationAveraging1DSFM", "TranslationAveragingBase"]
