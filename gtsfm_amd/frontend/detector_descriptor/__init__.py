"""Detector-descriptor plugins. The classes are exported lazily, so importing one plugin's module does not import the
others'."""
import importlib

_EXPORTS = {
    "SIFTDetectorDescriptor": "sift",
    "SuperPointDetectorDescriptor": "superpoint",
    "D2NetDetDesc": "d2net",
}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        return getattr(importlib.import_module(f"{__name__}.{_EXPORTS[name]}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
