"""eval_one_epoch (tools/eval_utils/eval_utils.py:52-140 of the reference): a detector over a loader in eval mode -> the
reference's ret_dict of recall/roi_*, recall/rcnn_* and the dataset's AP keys.

One process: det annos are neither pickled to a result directory nor merged across ranks (merge_results_dist); run it on one rank
over the whole loader. The 'Average/*' keys of the reference's add_avg_performance are not added."""
import torch

from ..datasets.synthetic_dataset import to_device_batch


def eval_one_epoch(cfg_or_post_cfg, model, dataloader, logger=None, output_path=None, **eval_kwargs):
    """cfg_or_post_cfg: a config with MODEL.POST_PROCESSING, or POST_PROCESSING itself (RECALL_THRESH_LIST is read).
    eval_kwargs go to dataset.evaluation (route=, PR_detail_dict=, detail=). -> ret_dict"""
    post = cfg_or_post_cfg
    if 'MODEL' in post:
        post = post['MODEL']
    if 'POST_PROCESSING' in post:
        post = post['POST_PROCESSING']
    thresh_list = list(post['RECALL_THRESH_LIST'])
    metric = {'gt_num': 0}
    for t in thresh_list:
        metric['recall_roi_%s' % str(t)] = metric['recall_rcnn_%s' % str(t)] = 0
    dataset = dataloader.dataset
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    det_annos = []
    try:
        for batch in dataloader:
            batch = to_device_batch(batch, device)
            with torch.no_grad():
                pred_dicts, recall = model(batch)
            for t in thresh_list:
                metric['recall_roi_%s' % str(t)] += recall.get('roi_%s' % str(t), 0)
                metric['recall_rcnn_%s' % str(t)] += recall.get('rcnn_%s' % str(t), 0)
            metric['gt_num'] += recall.get('gt', 0)
            det_annos += dataset.generate_prediction_dicts(batch, pred_dicts, dataset.class_names, output_path=output_path)
    finally:
        model.train(was_training)
    ret_dict = {}
    for t in thresh_list:
        ret_dict['recall/roi_%s' % str(t)] = metric['recall_roi_%s' % str(t)] / max(metric['gt_num'], 1)
        ret_dict['recall/rcnn_%s' % str(t)] = metric['recall_rcnn_%s' % str(t)] / max(metric['gt_num'], 1)
        if logger is not None:
            logger.info('recall_roi_%s: %f' % (t, ret_dict['recall/roi_%s' % str(t)]))
            logger.info('recall_rcnn_%s: %f' % (t, ret_dict['recall/rcnn_%s' % str(t)]))
    if logger is not None:
        logger.info('Average predicted number of objects(%d samples): %.3f'
                    % (len(det_annos), sum(len(a['name']) for a in det_annos) / max(1, len(det_annos))))
    result_str, result_dict = dataset.evaluation(det_annos, dataset.class_names, **eval_kwargs)
    if logger is not None:
        logger.info(result_str)
    ret_dict.update(result_dict)
    return ret_dict
