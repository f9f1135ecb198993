"""granne_amd -- MI355X-native search path for granne (Granne::search on gfx950).

Host-side mirror of the reference's Python interface (py/src/lib.rs: classes Granne and
GranneBuilder, function compute_distance) over the C ABI in include/granne_hip.h.
"""
from ._lib import F16, F32, I8, UNUSED, GranneHipError  # noqa: F401
from .index import Granne, compute_distance, from_f16, normalize, quantize, to_f16  # noqa: F401
from .builder import GranneBuilder  # noqa: F401
from .embeddings import SumEmbeddings  # noqa: F401
from .rw_builder import RwGranneBuilder  # noqa: F401
from .refined import RefinedGranne  # noqa: F401
from .filters import Filter  # noqa: F401

__all__ = ["Granne", "GranneBuilder", "RwGranneBuilder", "RefinedGranne", "Filter", "SumEmbeddings", "compute_distance", "normalize", "quantize", "to_f16", "from_f16", "GranneHipError", "F32", "I8", "F16", "UNUSED"]
