"""MI355X-native denoising hot path of LabJunBMI/E3-invaraint-diffusion-model.

Sub-packages mirror the reference's two script directories (same file names, entry points,
tensor layouts and checkpoint keys); the compute runs in hand-written gfx950 HIP kernels behind
the C-ABI of include/e3d_hip.h (csrc/, loaded by hip.py).  No CPU fallback.
"""
from . import hip  # noqa: F401

__all__ = ["hip", "ops", "bert", "blocks", "training", "optim", "sharding", "autograd", "biolip", "featurize", "evaluate", "packing", "design", "similarity", "structure_model", "sequence_model", "DesignControls", "score_sequences", "score_structures"]


def __getattr__(name):
    if name == "score_sequences":       # sequence_model/sample.py's, under the package's own name too
        from .sequence_model.sample import score_sequences
        return score_sequences
    if name == "score_structures":      # structure_model/sample.py's, next to it
        from .structure_model.sample import score_structures
        return score_structures
    if name == "DesignControls":        # the record of design.py, under the package's own name too
        from .design import DesignControls
        return DesignControls
    if name in __all__:
        import importlib
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(name)
