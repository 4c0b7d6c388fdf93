"""MI355X-native simplex pivot engine behind the solver surface of LPR_381_Group_V22.

Importing this package loads ``_lib/liblpr_engine.so`` (hand-written HIP for gfx950, built by
``__graft_entry__.build()``); there is no CPU fallback.
"""
from . import _native
from .engine import Engine, RevisedState, Tableau, default_engine
from .bb_batch import (BranchAndBoundBatch, option3_texts, solve_integer_programs,
                       write_option3_files)
from .branch_and_bound import (BranchAndBoundAdapter, BranchBoundTree, Comm,
                               solve_level_sync_native, solve_level_synchronous,
                               torch_collectives)
from .cut_batch import (CuttingPlaneBatch, cutting_plane_texts, format_cutting_plane,
                        pack_tableaux)
from .input_file_parser import Constraint, InputFileParser
from .knapsack import KnapsackBranchBoundSimplex, KnapsackBranchBoundSolver
from .knapsack_batch import KnapsackBatch, pack_knapsacks, solve_knapsacks
from .primal_batch import PrimalSimplexBatch, pack_models
from .primal_simplex_solver import PrimalSimplexSolver
from .revised_batch import RevisedSimplexBatch, pack_revised_models
from .revised_primal_simplex_solver import RevisedPrimalSimplexSolver, SolverException
from .sens_batch import (SensitivityBatch, SensitivityGrowBatch, SensitivityModelBatch,
                         optimal_items, pack_grow_scripts, pack_scripts)

__all__ = [
    "Engine", "Tableau", "default_engine", "Constraint", "InputFileParser",
    "PrimalSimplexSolver", "RevisedPrimalSimplexSolver", "RevisedState", "SolverException",
    "BranchAndBoundAdapter", "BranchBoundTree", "solve_level_synchronous", "torch_collectives",
    "Comm", "solve_level_sync_native", "KnapsackBranchBoundSimplex", "KnapsackBranchBoundSolver",
    "PrimalSimplexBatch", "pack_models", "BranchAndBoundBatch", "solve_integer_programs",
    "option3_texts", "write_option3_files",
    "SensitivityBatch", "SensitivityGrowBatch", "pack_scripts", "pack_grow_scripts",
    "SensitivityModelBatch", "optimal_items",
    "CuttingPlaneBatch", "pack_tableaux", "cutting_plane_texts", "format_cutting_plane",
    "KnapsackBatch", "pack_knapsacks", "solve_knapsacks",
    "RevisedSimplexBatch", "pack_revised_models",
    "_native",
]
