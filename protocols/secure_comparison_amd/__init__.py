"""MI355X-native batched secure comparison (DGK/Veugen protocol): the Paillier / DGK arithmetic underneath
Initiator.step_* and KeyHolder.step_* as hand-written HIP kernels behind a C ABI (libsc_amd.so)."""
from .aggregate import (cumsum_planes_batch, cumsum_rows_batch, secure_cdf_batch, secure_groupby_count_batch, secure_groupby_mean_batch,
                        secure_groupby_sum_batch, secure_histogram_batch, secure_histogram_median_batch, secure_majority_batch,
                        secure_quantile_batch, sum_planes_batch, sum_rows_batch)
from .communicator import Communicator, InMemoryCommunicator, StreamCommunicator
from .division import (DivDraws, DivLayout, draw_div, secure_divide_batch, secure_divmod_batch, secure_modulo_batch, secure_shift_right_batch)
from .dotproduct import (DotDraws, DotLayout, draw_dot, secure_dot_batch, secure_squared_distance_batch, secure_sum_squares_batch)
from .initiator import AlicePlain, Initiator
from .keyholder import BobPlain, KeyHolder
from .linear import linear_planes_batch, linear_rows_batch
from .lookup import OnehotDraws, OnehotLayout, draw_onehot, secure_gather_batch, secure_lookup_batch, secure_onehot_batch
from .multiplication import (MulDraws, MulLayout, draw_mul, secure_and_batch, secure_equal_batch, secure_in_range_batch, secure_multiply_batch,
                             secure_or_batch, secure_xor_batch)
from .schemes import DGK, DGKCiphertext, Paillier, PaillierCiphertext
from .selection import secure_argmax_batch, secure_argmin_batch, secure_maximum_batch, secure_minimum_batch
from .sorting import secure_kth_batch, secure_median_batch, secure_sort_batch, secure_topk_batch
from .utils import from_bits, to_bits

__all__ = ["linear_planes_batch", "linear_rows_batch", "sum_planes_batch", "sum_rows_batch", "cumsum_planes_batch", "cumsum_rows_batch", "secure_cdf_batch", "secure_quantile_batch",
           "secure_histogram_median_batch", "secure_histogram_batch", "secure_majority_batch", "secure_groupby_count_batch",
           "secure_groupby_sum_batch", "Communicator", "InMemoryCommunicator", "StreamCommunicator", "Initiator", "KeyHolder", "from_bits", "to_bits", "Paillier", "PaillierCiphertext", "DGK",
           "DGKCiphertext", "AlicePlain", "BobPlain", "secure_minimum_batch", "secure_maximum_batch", "secure_argmin_batch", "secure_argmax_batch",
           "secure_sort_batch", "secure_topk_batch", "secure_kth_batch", "secure_median_batch", "MulLayout", "MulDraws", "draw_mul",
           "secure_multiply_batch", "secure_and_batch", "secure_or_batch", "secure_xor_batch", "secure_equal_batch", "secure_in_range_batch",
           "DotLayout", "DotDraws", "draw_dot", "secure_dot_batch", "secure_sum_squares_batch", "secure_squared_distance_batch",
           "OnehotLayout", "OnehotDraws", "draw_onehot", "secure_onehot_batch", "secure_gather_batch", "secure_lookup_batch",
           "DivLayout", "DivDraws", "draw_div", "secure_divide_batch", "secure_modulo_batch", "secure_divmod_batch", "secure_shift_right_batch",
           "secure_groupby_mean_batch"]
__version__ = "0.1.0"
