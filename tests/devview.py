"""Zero-copy torch views of device memory the engine owns (test infrastructure only)."""


class DevArray:
    """zero-copy view of a device int32 array for torch.as_tensor (__cuda_array_interface__)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i4", "data": (int(ptr), False), "version": 2}
