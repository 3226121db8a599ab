"""``_target_: train_unconditional.TrainUnconditional`` resolves here (config/train_tshirt_mnist.yaml task._target_)."""
from siss_amd.tasks import TrainUnconditional  # noqa: F401
