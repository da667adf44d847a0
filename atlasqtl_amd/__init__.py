"""atlasqtl_amd -- MI355X-native variational-inference hot path of atlasqtl.

Public surface mirrors the reference package's exports for this path
(NAMESPACE:3-10): atlasqtl, set_hyper, set_init, assign_bFDR, summary and
print_atlasqtl (the S3 methods summary.atlasqtl / print.atlasqtl); plus the operator-level
coreDualLoop / coreDualMisLoop (R/RcppExports.R) backed by libatlasqtl_hip.so.
"""
from .api import add_collinear_back_pairs_, atlasqtl, print_atlasqtl, summary  # noqa: F401
from .core import (VbRun, assign_bFDR, associations, atlasqtl_global_core_, atlasqtl_global_local_core_,  # noqa: F401
                   coreDualLoop, coreDualMisLoop, hotspot_sizes, merge_pair_tables, value_summary)
from .hyper_init import set_hyper, set_init  # noqa: F401
from .checks import AtlasqtlError  # noqa: F401
from .prepare import genotype_grm, genotype_pcs, rank_normalize  # noqa: F401
from .plink import PlinkBed  # noqa: F401
from .marginal import marginal_screen  # noqa: F401
from .cis import cis_screen, cis_windows  # noqa: F401
from .cis_condition import cis_independent, independent_signals_  # noqa: F401
from .cis_susie import cis_finemap, credible_sets_  # noqa: F401
from .prediction import predict  # noqa: F401

__all__ = ["atlasqtl", "set_hyper", "set_init", "coreDualLoop", "coreDualMisLoop", "atlasqtl_global_local_core_", "atlasqtl_global_core_",
           "VbRun", "AtlasqtlError", "assign_bFDR", "hotspot_sizes", "associations", "merge_pair_tables",
           "add_collinear_back_pairs_", "summary", "print_atlasqtl", "value_summary", "PlinkBed", "genotype_grm",
           "genotype_pcs", "rank_normalize", "marginal_screen", "predict", "cis_screen", "cis_windows",
           "cis_independent", "independent_signals_", "cis_finemap", "credible_sets_"]
