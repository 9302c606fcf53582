from .device_mapper import DevicePartDistillationMapper, DeviceProposalMapper  # noqa: F401
from .gt_part_mapper import DeviceCityscapesPartMapper, DeviceGTPartMapper, DeviceVOCPartsMapper  # noqa: F401
