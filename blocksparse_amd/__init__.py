"""blocksparse_amd -- MI355X-native block-sparse matmul engine (drop-in for the BlocksparseMatMul hot path
of openai/blocksparse).  Host mirror of the reference operator interface over libbsmm_hip.so."""
from .lut import build_tables, z_order_2d, ceil_div  # noqa: F401
from .matmul import BlocksparseMatMul  # noqa: F401
from .transformer import BlocksparseTransformer  # noqa: F401
from .sparse_proj import SparseProj  # noqa: F401
from . import checkpoint  # noqa: F401
from . import sparsity  # noqa: F401
from .sparsity import blocksparse_norm, blocksparse_l2_decay, blocksparse_prune  # noqa: F401
from . import norms  # noqa: F401
from .norms import layer_norm  # noqa: F401
from . import ewops  # noqa: F401
from .ewops import bias_relu, fast_gelu, dropout, bias_dropout, set_entropy  # noqa: F401
from . import embed  # noqa: F401
from .embed import embedding_lookup  # noqa: F401
from . import xent  # noqa: F401
from .xent import softmax_cross_entropy  # noqa: F401
from . import lstm  # noqa: F401
from .lstm import fused_lstm_gates  # noqa: F401
from . import select  # noqa: F401
from .select import rectified_top_k, masked_top_k_softmax, masked_softmax, softmax, sparse_relu, select_path  # noqa: F401
from . import quantize  # noqa: F401  (the operator of the same name stays inside the module: blocksparse_amd.quantize.quantize)
from .quantize import QuantizeSpec, QuantizeState, log_stats, quantize_fwd, quantize_update_emax, tensor_stats  # noqa: F401
from .quantize import reset_quantize_states  # noqa: F401
from . import optimize  # noqa: F401
from .optimize import AdamOptimizer, Ema, PreparedStep, adam_step, ema_step, clip_by_global_norm, global_norm  # noqa: F401
from .optimize import AdafactorOptimizer, adafactor_step, adafactor_decay  # noqa: F401

__version__ = "0.1.0"
