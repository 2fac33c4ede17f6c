"""MI355X-native GP-posterior + acquisition engine for bayes_opt's suggest() hot path.

Hand-written HIP (gfx950) behind a C ABI (include/gpbo.h, include/gpmo.h), loaded with ctypes.  No PyTorch, no
Triton, no CPU fallback: importing the host classes works anywhere, creating an engine requires the
built library and an AMD GPU.
"""
__version__ = "0.1.0"

__all__ = ["GpEngine", "HipGPR", "HipConstraintModel", "FloatSpace", "accelerate", "suggest_batch", "UpperConfidenceBound",
           "ExpectedImprovement", "ProbabilityOfImprovement", "LogExpectedImprovement", "LogConstrainedExpectedImprovement",
           "suggest_thompson",
           "suggest_mes", "suggest_kg", "suggest_turbo", "TrustRegion", "sobol_tables",
           "suggest_constrained_thompson", "suggest_scbo", "ConstrainedTrustRegion",
           "ParetoOptimizer", "pareto_front", "hypervolume", "box_decomposition", "suggest_qnei", "suggest_qnehvi",
           "suggest_constrained_qnei", "suggest_constrained_qnehvi"]


def __getattr__(name):  # lazy: `import bayesianoptimization_amd.workloads` must not need sklearn/scipy
    if name == "GpEngine":
        from .engine import GpEngine
        return GpEngine
    if name == "HipGPR":
        from .gpr import HipGPR
        return HipGPR
    if name == "HipConstraintModel":
        from .constraint_model import HipConstraintModel
        return HipConstraintModel
    if name == "FloatSpace":
        from .float_space import FloatSpace
        return FloatSpace
    if name == "accelerate":
        from .dropin import accelerate
        return accelerate
    if name == "suggest_batch":
        from .batch import suggest_batch
        return suggest_batch
    if name == "suggest_thompson":
        from .thompson import suggest_thompson
        return suggest_thompson
    if name == "suggest_mes":
        from .mes import suggest_mes
        return suggest_mes
    if name == "suggest_kg":
        from .kg import suggest_kg
        return suggest_kg
    if name in ("suggest_turbo", "TrustRegion", "sobol_tables"):
        from . import turbo
        return getattr(turbo, name)
    if name in ("suggest_constrained_thompson", "suggest_scbo", "ConstrainedTrustRegion"):
        from . import scbo
        return getattr(scbo, name)
    if name in ("ParetoOptimizer", "pareto_front", "hypervolume", "box_decomposition"):
        from . import multiobjective
        return getattr(multiobjective, name)
    if name == "suggest_qnei":
        from .qnei import suggest_qnei
        return suggest_qnei
    if name == "suggest_constrained_qnei":
        from .cqnei import suggest_constrained_qnei
        return suggest_constrained_qnei
    if name == "suggest_constrained_qnehvi":
        from .cqnehvi import suggest_constrained_qnehvi
        return suggest_constrained_qnehvi
    if name == "suggest_qnehvi":
        from .qnehvi import suggest_qnehvi
        return suggest_qnehvi
    if name in ("UpperConfidenceBound", "ExpectedImprovement", "ProbabilityOfImprovement", "LogExpectedImprovement",
                "LogConstrainedExpectedImprovement",
                "AcquisitionFunction"):
        from . import fused_acquisition as acquisition
        return getattr(acquisition, name)
    raise AttributeError(name)
