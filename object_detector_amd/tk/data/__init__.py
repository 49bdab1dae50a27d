from . import coco, voc  # noqa: F401
