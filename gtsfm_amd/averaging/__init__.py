"""Averaging stages of the reference pipeline (gtsfm/averaging)."""
