"""libflagstats_amd -- MI355X (gfx950) engine for libflagstats' flagstat hot path.

Only what the path needs:

* ``csrc/``          hand-written HIP kernels + the C-ABI shim -> ``libflagstats_hip.so``
                     (declared in ``include/libflagstats_hip.h``)
* ``pyflagstats``    mirror of the reference's Python entry point
                     (``python/libflagstats.pyx``): ``flagstats(values)``
* ``device``         device-resident arrays, on-device input makers, torch interop
* ``segments``       per-segment counters (CSR offsets) in one launch: host arrays,
                     device pointers, torch tensors
* ``wide``           the same counters for int32 / int64 (and 16-bit) arrays and tensors,
                     with the mask of bits seen above bit 15
* ``where``          the same counters for the elements a boolean mask or an LSB-first
                     bitmap selects, with the number selected, in one pass
* ``filter``         the same counters for the reads that pass samtools' ``-f`` / ``-F`` / ``-q``
                     (FLAG bits required and excluded, a MAPQ threshold), with no mask array
* ``filter_rf``      the filter with the rest of samtools' FLAG predicate, ``--rf`` (at least one of these bits) and ``-G``
                     (not all of these bits), on ``uint16`` arrays as a whole
* ``filter_where``   the filter and a boolean mask or bitmap together: the counters of the reads that pass ``-f`` / ``-F`` /
                     ``-q`` AND are selected (the non-null rows of an Arrow FLAG column), with their number, in one pass
* ``segments_filter`` the filter per segment: rows of counters and the number of reads that pass, for
                     every CSR segment in one launch
* ``segments_filter_rf`` ``segments_filter`` under samtools' whole FLAG predicate: ``--rf`` (at least one of these bits) and
                     ``-G`` (not all of these bits) per segment of a ``uint16`` array, for every CSR segment in one launch
* ``segments_where`` the mask or bitmap per segment: rows of counters and the number of selected reads, for every CSR
                     segment in one launch (the selection is indexed by array element)
* ``segments_filter_where`` the filter and the mask or bitmap together per segment: rows of counters and the number of reads
                     that pass AND are selected, for every CSR segment in one launch
* ``wide_filter``    the filter on int32 / int64 (and 16-bit) arrays and tensors in place: counters, the number of
                     reads that pass and the mask of bits seen above bit 15, in one pass
* ``wide_filter_rf`` ``wide_filter`` under samtools' whole FLAG predicate: ``--rf`` (at least one of these bits) and ``-G``
                     (not all of these bits) on int32 / int64 (and 16-bit) arrays and tensors in place, as a whole
* ``wide_where``     the mask or bitmap on int32 / int64 (and 16-bit) arrays and tensors in place: counters, the number
                     selected and the mask of bits seen above bit 15 of the selected elements, in one pass
* ``wide_filter_where`` the filter and the mask or bitmap together on int32 / int64 (and 16-bit) arrays and tensors in place:
                     counters, the number of reads that pass AND are selected and the mask of bits seen above bit 15 of the
                     selected elements, in one pass
* ``segments_wide``  rows of counters and one high-bit mask per CSR segment of an int32 / int64 (or 16-bit) array or
                     tensor, in one launch
* ``segments_wide_filter`` the filter per segment of an int32 / int64 (or 16-bit) array or tensor in place: rows of counters,
                     the number of reads that pass and one high-bit mask per CSR segment, in one launch
* ``segments_wide_where`` the mask or bitmap per segment of an int32 / int64 (or 16-bit) array or tensor in place: rows of
                     counters, the number selected and one high-bit mask of the selected elements per CSR segment, in one launch
* ``segments_wide_filter_where`` the filter and the mask or bitmap together per segment of an int32 / int64 (or 16-bit) array or
                     tensor in place: rows of counters, the number of reads that pass AND are selected and one high-bit mask of
                     the selected elements per CSR segment, in one launch
* ``dist``          shard + single all-reduce for multi-GPU runs

The hot path has no CPU fallback: importing the compute entry points without the
built extension raises.
"""
from .pyflagstats import SAM_FLAG_NAMES, flagstats, flagstats_x64  # noqa: F401
from .segments import (  # noqa: F401
    count_segments_device_ptr,
    count_segments_torch,
    flagstats_segments,
    offsets_from_lengths,
    segment_dicts,
)
from .filter import count_device_ptr_filter, count_torch_filter, counters_filter, flagstats_filter  # noqa: F401
from .filter_rf import (  # noqa: F401
    count_device_ptr_filter_rf,
    count_torch_filter_rf,
    counters_filter_rf,
    flagstats_filter_rf,
)
from .filter_where import (  # noqa: F401
    count_device_ptr_filter_where,
    count_torch_filter_where,
    counters_filter_where,
    flagstats_filter_where,
)
from .segments_filter import (  # noqa: F401
    count_segments_device_ptr_filter,
    count_segments_torch_filter,
    flagstats_segments_filter,
    segment_filter_dicts,
)
from .segments_filter_rf import (  # noqa: F401
    count_segments_device_ptr_filter_rf,
    count_segments_torch_filter_rf,
    flagstats_segments_filter_rf,
)
from .segments_wide import (  # noqa: F401
    count_segments_device_ptr_ints,
    count_segments_torch_ints,
    counters_segments_ints,
    flagstats_segments_ints,
)
from .segments_wide_filter import (  # noqa: F401
    count_segments_device_ptr_ints_filter,
    count_segments_torch_ints_filter,
    counters_segments_ints_filter,
    flagstats_segments_ints_filter,
)
from .segments_where import (  # noqa: F401
    count_segments_device_ptr_where,
    count_segments_torch_where,
    counters_segments_where,
    flagstats_segments_where,
)
from .segments_filter_where import (  # noqa: F401
    count_segments_device_ptr_filter_where,
    count_segments_torch_filter_where,
    counters_segments_filter_where,
    flagstats_segments_filter_where,
)
from .segments_wide_filter_where import (  # noqa: F401
    count_segments_device_ptr_ints_filter_where,
    count_segments_torch_ints_filter_where,
    counters_segments_ints_filter_where,
    flagstats_segments_ints_filter_where,
)
from .segments_wide_where import (  # noqa: F401
    count_segments_device_ptr_ints_where,
    count_segments_torch_ints_where,
    counters_segments_ints_where,
    flagstats_segments_ints_where,
)
from .where import count_device_ptr_where, count_torch_where, counters_where, flagstats_where  # noqa: F401
from .wide import count_device_ptr_ints, count_torch_ints, counters_ints, flagstats_ints  # noqa: F401
from .wide_filter import (  # noqa: F401
    count_device_ptr_ints_filter,
    count_torch_ints_filter,
    counters_ints_filter,
    flagstats_ints_filter,
)
from .wide_filter_rf import (  # noqa: F401
    count_device_ptr_ints_filter_rf,
    count_torch_ints_filter_rf,
    counters_ints_filter_rf,
    flagstats_ints_filter_rf,
)
from .wide_filter_where import (  # noqa: F401
    count_device_ptr_ints_filter_where,
    count_torch_ints_filter_where,
    counters_ints_filter_where,
    flagstats_ints_filter_where,
)
from .wide_where import (  # noqa: F401
    count_device_ptr_ints_where,
    count_torch_ints_where,
    counters_ints_where,
    flagstats_ints_where,
)

__all__ = ["flagstats", "flagstats_x64", "SAM_FLAG_NAMES", "flagstats_segments", "offsets_from_lengths",
           "count_segments_device_ptr", "count_segments_torch", "segment_dicts", "counters_ints", "flagstats_ints",
           "count_device_ptr_ints", "count_torch_ints", "counters_where", "flagstats_where", "count_device_ptr_where",
           "count_torch_where", "counters_filter", "flagstats_filter", "count_device_ptr_filter", "count_torch_filter",
           "flagstats_segments_filter", "count_segments_device_ptr_filter", "count_segments_torch_filter", "segment_filter_dicts",
           "counters_ints_filter", "flagstats_ints_filter", "count_device_ptr_ints_filter", "count_torch_ints_filter",
           "counters_segments_ints", "flagstats_segments_ints", "count_segments_device_ptr_ints", "count_segments_torch_ints",
           "counters_segments_ints_filter", "flagstats_segments_ints_filter", "count_segments_device_ptr_ints_filter",
           "count_segments_torch_ints_filter", "counters_segments_where", "flagstats_segments_where",
           "count_segments_device_ptr_where", "count_segments_torch_where", "counters_ints_where", "flagstats_ints_where",
           "count_device_ptr_ints_where", "count_torch_ints_where", "counters_segments_ints_where", "flagstats_segments_ints_where",
           "count_segments_device_ptr_ints_where", "count_segments_torch_ints_where", "counters_filter_where",
           "flagstats_filter_where", "count_device_ptr_filter_where", "count_torch_filter_where",
           "counters_segments_filter_where", "flagstats_segments_filter_where", "count_segments_device_ptr_filter_where",
           "count_segments_torch_filter_where", "counters_ints_filter_where", "flagstats_ints_filter_where",
           "count_device_ptr_ints_filter_where", "count_torch_ints_filter_where", "counters_segments_ints_filter_where",
           "flagstats_segments_ints_filter_where", "count_segments_device_ptr_ints_filter_where",
           "count_segments_torch_ints_filter_where", "counters_filter_rf", "flagstats_filter_rf", "count_device_ptr_filter_rf",
           "count_torch_filter_rf", "counters_ints_filter_rf", "flagstats_ints_filter_rf", "count_device_ptr_ints_filter_rf",
           "count_torch_ints_filter_rf", "flagstats_segments_filter_rf", "count_segments_device_ptr_filter_rf",
           "count_segments_torch_filter_rf"]
