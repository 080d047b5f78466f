from .registry import (EnvSpec, get_spec, host_spec, known_envs, register_tensor_env, import_env_module,
                       kernel_kind_of, KIND_CARTPOLE, KIND_HOST, KIND_PENDULUM, KIND_SYNTHETIC, KIND_TENSOR)
from .vec_env import VecEnv, SyntheticEnv, PendulumEnv, CartPoleContinuousEnv, make_vec_env
from .gym_adapter import GymVecEnv, gym_available, register_env

__all__ = ["EnvSpec", "get_spec", "host_spec", "known_envs", "KIND_CARTPOLE", "KIND_HOST", "KIND_PENDULUM",
           "KIND_SYNTHETIC", "KIND_TENSOR", "register_tensor_env", "import_env_module", "kernel_kind_of",
           "VecEnv", "SyntheticEnv", "PendulumEnv", "CartPoleContinuousEnv", "make_vec_env", "GymVecEnv",
           "gym_available", "register_env"]
