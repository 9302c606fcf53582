from .cityscapes_part_record import cityscapes_part_records, load_object_and_parts  # noqa: F401
from .device_mapper import DevicePartDistillationMapper, DeviceProposalMapper  # noqa: F401
from .gt_part_mapper import DeviceCityscapesPartMapper, DeviceGTPartMapper, DeviceVOCPartsMapper  # noqa: F401
from .part_imagenet_mapper import DevicePartImageNetMapper  # noqa: F401
from .imagenet_stage_mapper import (DeviceImagenetPartRankingMapper, DeviceProposalGenerationMapper, imagenet_proposal_record,  # noqa: F401
                                    imagenet_record)
