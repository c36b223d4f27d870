"""bayesiannetwork_amd -- MI355X-native Loopy Belief Propagation / Likelihood Weighting.

Host-side mirror of the reference's ``bn::inference`` functors over hand-written HIP kernels
(``csrc/``) behind the C ABI declared in ``include/bn_mi355x.h``.  The HIP library is loaded on
first use and its absence is a hard error: there is no CPU fallback in this package.
"""
from .flat import Evidence, FlatModel, from_parent_lists  # noqa: F401
from . import synth  # noqa: F401

_EVALUATION = ("AIC", "MDL", "log_cpt", "log_likelihood_nodes", "log_likelihood_rows", "parameters", "ci_tests", "chisq_sf")
_LEARNING = ("Greedy", "K2", "Learner", "score_groups", "score_subsets", "BruteForce", "StepwiseStructure", "TermTable",
             "SimulatedAnnealing", "StepwiseStructureHC", "HillClimbing", "OptimalSearch", "PC", "PCResult", "cpdag_to_dag")
_EM = ("MISSING", "em_expected_counts", "em_fit", "jt_em_fit")
_INFERENCE = ("GibbsSampling",)
__all__ = ["Evidence", "FlatModel", "from_parent_lists", "synth", *_EVALUATION, *_LEARNING, *_EM, *_INFERENCE]


def __getattr__(name):
    # the scores of evaluation.py, resolved at first use: importing the package alone loads neither the ctypes loader nor the library
    if name in _EVALUATION:
        from . import evaluation
        return getattr(evaluation, name)
    if name in _LEARNING:
        from . import learning
        return getattr(learning, name)
    if name in _EM:   # expectation-maximisation (engine.py): CPTs from a table with unobserved cells
        from . import engine
        return getattr(engine, name)
    if name in _INFERENCE:   # Gibbs sampling (engine.py), beside engine.LikelihoodWeighting
        from . import engine
        return getattr(engine, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
