from .mlp_dynamics import MLPDynamicsModel  # noqa: F401
from .meta_mlp_dynamics import MetaMLPDynamicsModel  # noqa: F401
from .rnn_dynamics import RNNDynamicsModel, LSTMStateTuple  # noqa: F401
from .reward_model import MLPRewardModel  # noqa: F401
from .value_model import MLPValueModel  # noqa: F401
from .policy_model import MLPPolicyModel  # noqa: F401
