/* rkfd_reset_host.h - rkfd_capi_reset.hip as rkfd_capi.hip sees it: the bank of start states of one batch, the staging of a host
 * array of slot values and the launch of rkfd_reset_kernel, behind rkfdBatchBankReserve / BankStore / Reset / ResetDev.  The caller
 * has selected the device and - for the synchronous calls (reserve, store, rows) - waited for the batch's launches.  Failures
 * return -1 with a message in err. */
#ifndef RKFD_RESET_HOST_H
#define RKFD_RESET_HOST_H

#include "rkfd_model.h"
#include "rkfd_devmodel.h"

#define RKFD_RESET_MAX_PARTS 8      /* parts of a split launch that stage their own block of the slot values (RKFD_MAX_SPLIT) */

struct rkfdReset;
/* batch instances of ND joint coordinates, NL links and NC contact candidates; allocates nothing on the device */
extern "C" rkfdReset *rkfd_reset_create(int batch, int ND, int NL, int NC, char *err, int errlen);
extern "C" void rkfd_reset_destroy(rkfdReset *r);
/* (re)allocates the bank with nslots rows, contents undefined; 0 frees it */
extern "C" int rkfd_reset_reserve(rkfdReset *r, int nslots, char *err, int errlen);
extern "C" int rkfd_reset_size(const rkfdReset *r);
/* rows slot .. slot+count-1 of the bank <- rows first .. first+count-1 of st (device to device), complete when it returns */
extern "C" int rkfd_reset_store(rkfdReset *r, const rkfdDevState *st, int slot, int first, int count, char *err, int errlen);
/* the node level's route through the host: bytes of `count` packed rows; rows first .. of st into buf; buf into rows slot .. of the bank */
extern "C" size_t rkfd_reset_row_bytes(const rkfdReset *r, int count);
extern "C" int rkfd_reset_rows_get(rkfdReset *r, const rkfdDevState *st, int first, int count, void *buf, char *err, int errlen);
extern "C" int rkfd_reset_rows_put(rkfdReset *r, int slot, int count, const void *buf, char *err, int errlen);
/* a host array slots[batch] into the pinned staging (waits for the launches of the previous call that read the batch's copy first);
 * then, per part [lo, hi) and on the stream that part runs on, the upload of its block to the batch's device copy, followed by
 * rkfd_reset_launch over the same part with that copy - `part` (0 .. RKFD_RESET_MAX_PARTS-1) names the event that marks the end of
 * the pair.  rkfd_reset_dev_slots: the device copy (NULL before the first stage) */
extern "C" int rkfd_reset_stage(rkfdReset *r, const int *slots, char *err, int errlen);
extern "C" int rkfd_reset_upload(rkfdReset *r, int lo, int hi, int part, void *stream, char *err, int errlen);
extern "C" const int *rkfd_reset_dev_slots(const rkfdReset *r);
/* one launch of rkfd_reset_kernel over the instances [lo, hi) on `stream`: slots_dev[batch] on the device; snap: the whole-batch
 * snapshot or NULL when none was taken */
extern "C" int rkfd_reset_launch(rkfdReset *r, const rkfdDevState *st, const rkfdDevState *snap, const int *slots_dev, int lo, int hi,
                                 int *errflag, void *stream, char *err, int errlen);

#endif /* RKFD_RESET_HOST_H */
