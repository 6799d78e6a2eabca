"""Unified inference interface (reference: src/quantized_sae/inference/)."""
from .framework import (  # noqa: F401
    SAE_REGISTRY,
    SAERegistryEntry,
    SAEWrapper,
    available_saes,
    compute_reconstruction_error,
    load_sae,
)
from .dictionary import compare_decoders, decoder_atoms, decoder_cosine_similarity  # noqa: F401,E402
from .inspector import DictionaryInspector, FeatureOverview, integer_atoms, nearest_atoms  # noqa: F401,E402
from .clustering import kmeans_atoms  # noqa: F401,E402
from .token_overlap import (  # noqa: F401,E402
    JaccardHistogram,
    TokenSets,
    average_unique_tokens_per_active_feature,
    jaccard_histogram,
    top_token_sets,
)
from .token_lists import TokenLists, token_lists_to_python  # noqa: F401,E402
from .top_examples import TopExamples, examples_to_python  # noqa: F401,E402
from .coactivation_partners import CoactivationPartners  # noqa: F401,E402
from .evaluation import (  # noqa: F401,E402
    DatasetMoments,
    estimate_baseline_error,
    evaluate_dataset,
    format_quantization_report,
    quantization_error,
)
from .sparsity_curve import SparsityCurve, default_ks, sparsity_curve  # noqa: F401,E402
from .nested import nested_errors  # noqa: F401,E402
from .summary import (  # noqa: F401,E402
    average_coactivating_features,
    count_below_threshold,
    level_sizes,
    summarize_activation_counts,
    summarize_sae,
)
