from .device_mapper import DevicePartDistillationMapper, DeviceProposalMapper  # noqa: F401
