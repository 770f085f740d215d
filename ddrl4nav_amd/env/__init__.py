from ddrl4nav_amd.env.device_env import ENV_NAMES, DeviceEnv, make_device_env

__all__ = ["DeviceEnv", "make_device_env", "ENV_NAMES"]
