from .eval import get_official_eval_result, do_eval, eval_class, calculate_iou_partly  # noqa: F401
