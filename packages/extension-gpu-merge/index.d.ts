// Type declarations for @hocuspocus/extension-gpu-merge (see src/index.js).
import type { Extension, fetchPayload, storePayload, onLoadDocumentPayload, afterLoadDocumentPayload,
  onChangePayload, onStoreDocumentPayload, afterUnloadDocumentPayload } from '@hocuspocus/server'

export declare class YgmError extends Error {
  code: 'EMALFORMED' | 'ERANGE' | 'ENONCANON' | 'ESURROGATE' | 'EDEPTH' | 'ENOMEM' | 'EDEVICE' | 'EINVAL' | 'EUNSUPPORTED' | string
  status: number
}

/** A document's yDocOptions where the engine needs them: gc false marks a document created with { gc: false }
 *  (packages/server/src/types.ts:152-154, Hocuspocus.ts:331-344), whose snapshots and SyncStep2 replies keep deleted content. */
export interface DocOptions { gc?: boolean }
/** one option per document or state: an option byte (1 = no-GC), true (no-GC), or DocOptions; or the bytes themselves */
export type DocOptionList = ArrayLike<number | boolean | DocOptions> | Uint8Array

/** the fields of a document to serialize: null, undefined or [] for every key of doc.share, else their names */
export type FieldList = (string | Uint8Array)[] | null | undefined
export interface GpuEngineOptions {
  device?: number; compat135?: boolean; batchWindowMs?: number; maxBatchDocs?: number
  /** YGM_F_FLOATS (default false): jsonMany / jsonFieldsMany / toJsonMany, and jsonOf / versionJson / sharedJsonOf /
   *  versionSharedJson of the extension, write non-integer numbers (103.5, 1.5e-7, integers above 2^53) as JSON.stringify
   *  does instead of refusing the document with ENONCANON.  Still refused: JSON text with a number of more than 15
   *  significant digits or an exponent, BigInt, Uint8Array, __proto__, hashed mark names. */
  floats?: boolean
}

export declare class GpuEngine {
  constructor (opts?: GpuEngineOptions)
  mergeUpdates (updates: Uint8Array[]): Promise<Uint8Array>
  diffUpdate (update: Uint8Array, stateVector: Uint8Array): Promise<Uint8Array>
  encodeStateVectorFromUpdate (update: Uint8Array): Promise<Uint8Array>
  mergeMany (docs: Uint8Array[][]): Promise<(Uint8Array | YgmError)[]>
  diffMany (states: Uint8Array[], svs: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  stateVectorsMany (states: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  /** SyncStep2 payloads of stored documents: Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc(), state), sv) per pair */
  step2Many (states: Uint8Array[], svs: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** Many state vectors answered from shared states (a reconnect storm): ask a is answered from states[askState[a]] with
   *  svs[a]; one result per ask, in caller order, equal to diffMany / step2Many of the pair.  Each state is uploaded
   *  (step2Shared: and snapshotted) once.  An askState entry that names no state rejects with YgmError EINVAL. */
  diffShared (states: Uint8Array[], askState: ArrayLike<number>, svs: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  /** opts: one option per state; all of a state's asks are answered with it */
  step2Shared (states: Uint8Array[], askState: ArrayLike<number>, svs: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** update format V2: Y.mergeUpdatesV2 / Y.diffUpdateV2 / Y.encodeStateVectorFromUpdateV2 / Y.convertUpdateFormat* (yjs 13.6) */
  mergeManyV2 (docs: Uint8Array[][]): Promise<(Uint8Array | YgmError)[]>
  diffManyV2 (states: Uint8Array[], stateVectors: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  stateVectorsManyV2 (states: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  convertManyV1ToV2 (updates: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  convertManyV2ToV1 (updates: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  /** Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc(), update)) (doc-normalized snapshot, SURVEY.md §8f-1) */
  /** { gc: false }: Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc({ gc: false }), update)); both kinds share a batch window */
  snapshot (update: Uint8Array, opts?: DocOptions): Promise<Uint8Array>
  snapshotMany (states: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** Y.snapshotContainsUpdate(Y.snapshot(doc), update), states being normalized (snapshotMany) states */
  containsMany (states: Uint8Array[], updates: Uint8Array[]): Promise<(boolean | YgmError)[]>
  /** version history: Y.encodeSnapshot(Y.snapshot(doc)) of doc = Y.applyUpdate(new Y.Doc(), state); the single form shares a batch window */
  takeVersion (state: Uint8Array): Promise<Uint8Array>
  takeVersionMany (states: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  /** plain text of stored documents: doc.getText(names[i]).toString() of doc = Y.applyUpdate(new Y.Doc(), states[i]); deep:
   *  also descends into nested types (XmlFragment / Tiptap), one '\n' after each; an absent root name gives '' */
  textMany (states: Uint8Array[], names: (string | Uint8Array)[], opts?: { deep?: boolean }): Promise<(string | YgmError)[]>
  /** stored documents as ProseMirror / Tiptap JSON: JSON.stringify(TiptapTransformer.fromYdoc(doc, names[i])) of
   *  doc = Y.applyUpdate(new Y.Doc(), states[i]); a document outside the envelope gives a YgmError in its place */
  jsonMany (states: Uint8Array[], names: (string | Uint8Array)[]): Promise<(string | YgmError)[]>
  /** every asked field of stored documents as one JSON object: JSON.stringify(TiptapTransformer.fromYdoc(doc, fields[i])) of
   *  doc = Y.applyUpdate(new Y.Doc(), states[i]) -- a change webhook's `document`; fields[i]: null / [] for every key of
   *  doc.share, or the names; one load of a state serves all its fields; a refusing field or one named __proto__ gives a YgmError */
  jsonFieldsMany (states: Uint8Array[], fields: (FieldList)[]): Promise<(string | YgmError)[]>
  /** toJSON of stored Map / Array / Text roots: JSON.stringify(doc.getMap(names[i]).toJSON()) (kind TOJSON_MAP), getArray
   *  (TOJSON_ARRAY) or getText (TOJSON_TEXT) of doc = Y.applyUpdate(new Y.Doc(), states[i]); one kind per batch; a document
   *  outside the envelope (a nested Xml type, binary content, a non-integer number) gives a YgmError in its place */
  toJsonMany (states: Uint8Array[], names: (string | Uint8Array)[], kind: 0 | 1 | 2): Promise<(string | YgmError)[]>
  /** Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), new Y.Doc(opts))) of doc =
   *  Y.applyUpdate(new Y.Doc({ gc: false }), state); several versions of one document: restoreVersionShared */
  restoreVersion (state: Uint8Array, version: Uint8Array, opts?: DocOptions): Promise<Uint8Array>
  restoreVersionMany (states: Uint8Array[], versions: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** Many versions restored from shared states: ask a restores versions[a] from states[askState[a]]; one result per ask,
   *  in caller order, equal to restoreVersionMany of the pair.  Each state is uploaded and given its no-GC snapshot once.
   *  opts: one option per ask (the option belongs to the restored document).  An askState entry that names no state
   *  rejects with YgmError EINVAL. */
  restoreVersionShared (states: Uint8Array[], askState: ArrayLike<number>, versions: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** the context's counters (ygm_stats_t), camel-cased: calls, docs, kernelMs, h2dMs, d2hMs, hostSyncs, docsPending,
   *  docsSnapshot (documents the snapshot kernels ran on: one per state for step2Shared, one per pair for step2Many), ... */
  stats (): Record<string, number>
  close (): void
}

/** FNV-1a 64 of the UTF-8 document name: the device of a document is fnv1a64(name) % devices.length */
export declare function fnv1a64 (name: string): bigint

/** One GpuEngine per device; documents sharded by fnv1a64(documentName) mod N (SURVEY.md §8e). */
export declare class GpuEnginePool {
  constructor (opts?: GpuEngineOptions & { devices?: number[] })
  shardOf (documentName: string): number
  engineFor (documentName: string): GpuEngine
  mergeUpdates (updates: Uint8Array[], documentName?: string): Promise<Uint8Array>
  diffUpdate (update: Uint8Array, stateVector: Uint8Array, documentName?: string): Promise<Uint8Array>
  encodeStateVectorFromUpdate (update: Uint8Array, documentName?: string): Promise<Uint8Array>
  mergeMany (names: string[], docs: Uint8Array[][]): Promise<(Uint8Array | YgmError)[]>
  diffMany (names: string[], states: Uint8Array[], svs: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  stateVectorsMany (names: string[], states: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  step2Many (names: string[], states: Uint8Array[], svs: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** the shared-state forms, names[i] naming states[i]: states go to their fnv1a64(name) shard, results in ask order */
  diffShared (names: string[], states: Uint8Array[], askState: ArrayLike<number>, svs: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  step2Shared (names: string[], states: Uint8Array[], askState: ArrayLike<number>, svs: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  snapshot (update: Uint8Array, documentName?: string, opts?: DocOptions): Promise<Uint8Array>
  snapshotMany (names: string[], states: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  containsMany (names: string[], states: Uint8Array[], updates: Uint8Array[]): Promise<(boolean | YgmError)[]>
  takeVersionMany (names: string[], states: Uint8Array[]): Promise<(Uint8Array | YgmError)[]>
  /** docNames[i] routes states[i]; names[i] is its root name */
  textMany (docNames: string[], states: Uint8Array[], names: (string | Uint8Array)[], opts?: { deep?: boolean }): Promise<(string | YgmError)[]>
  jsonMany (docNames: string[], states: Uint8Array[], names: (string | Uint8Array)[]): Promise<(string | YgmError)[]>
  /** docNames[i] routes states[i]; fields[i] is its field list */
  jsonFieldsMany (docNames: string[], states: Uint8Array[], fields: (FieldList)[]): Promise<(string | YgmError)[]>
  /** docNames[i] routes states[i]; names[i] is its root name; kind as GpuEngine.toJsonMany's */
  toJsonMany (docNames: string[], states: Uint8Array[], names: (string | Uint8Array)[], kind: 0 | 1 | 2): Promise<(string | YgmError)[]>
  restoreVersionMany (names: string[], states: Uint8Array[], versions: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  /** names[i] naming states[i], routed as step2Shared; opts: one option per ask */
  restoreVersionShared (names: string[], states: Uint8Array[], askState: ArrayLike<number>, versions: Uint8Array[], opts?: DocOptionList): Promise<(Uint8Array | YgmError)[]>
  stats (): Record<string, number>[]
  /** node-wide totals: every per-device counter summed over the pool, plus `devices` */
  statsTotal (): Record<string, number>
  close (): void
}

/** Batched SyncStep1 -> SyncStep2 responder (SURVEY.md §8f-2; src/sync.js). */
export declare class SyncResponder {
  /** getDocOptions: a document's yDocOptions ({ gc: false }: its replies carry the deleted Items with their content); without it every document is garbage-collected */
  constructor (opts: { engine: GpuEngine | GpuEnginePool, getState: (documentName: string) => Promise<Uint8Array | Uint8Array[] | null>,
    getDocOptions?: (documentName: string) => DocOptions | null | undefined })
  /** per message: [Step2 reply, server Step1] for SyncStep1, null for other messages, an Error if malformed */
  answerMany (messages: Uint8Array[], opts?: { path?: 'connection' | 'reply' | 'none' }): Promise<(Uint8Array[] | Error | null)[]>
  /** read-only connections' SyncStep2 (MessageReceiver.ts:156-179): the SyncStatus(contained) frame per message */
  answerReadOnlyMany (messages: Uint8Array[]): Promise<(Uint8Array | Error | null)[]>
}

/** Batched Redis fan-out (SURVEY.md §8f-3; src/redis.js): extension-redis's per-change Step1 publishes and
 * remote SyncStep1 replies as GPU batches, with the reference's channel names and message framing. */
export declare class RedisFanout {
  constructor (opts: { engine: GpuEngine | GpuEnginePool, getState: (documentName: string) => Promise<Uint8Array | Uint8Array[] | null>,
    getDocOptions?: (documentName: string) => DocOptions | null | undefined,
    publish: (channel: string, message: Buffer) => any, identifier?: string, prefix?: string, windowMs?: number })
  identifier: string
  redisTransactionOrigin: string
  onChange (data: { documentName: string, transactionOrigin?: any }): Promise<void>
  /** null for own messages; answers SyncStep1 (replies published); otherwise the message for the host to apply */
  handleIncomingMessage (channel: string | Buffer, data: Buffer): Promise<null | { documentName: string | null, message?: Buffer, replied?: number }>
}

export declare class DocumentStore {
  fetchMany (payloads: fetchPayload[]): Promise<(Uint8Array | Uint8Array[] | null)[]>
  storeMany (entries: { payload: onStoreDocumentPayload; state: Buffer }[]): Promise<void>
  static fromDatabase (config: { fetch?: (p: fetchPayload) => Promise<Uint8Array | Uint8Array[] | null>; store?: (p: storePayload) => Promise<void> }): DocumentStore
}

export interface GpuMergeConfiguration extends GpuEngineOptions {
  /** several GPUs: documents sharded by fnv1a64(documentName) mod devices.length */
  devices?: number[]
  /** a batched DocumentStore, or the DatabaseConfiguration.store function (Database.ts:19) */
  store?: DocumentStore | ((p: storePayload) => Promise<void>)
  fetch?: (p: fetchPayload) => Promise<Uint8Array | Uint8Array[] | null>
  priority?: number
  engine?: GpuEngine
  Y?: any
  /** a refused merge: store Y.encodeStateAsUpdate(document) ('reference', default) or reject the store ('throw') */
  onRefused?: 'reference' | 'throw'
  /** store the GPU doc-normalized snapshot of the merge (GC'd, merged: the shape extension-database stores); default true, false stores the bare merge */
  normalize?: boolean
  /** merged states over this many bytes are stored as the bare merge (the snapshot kernel runs one thread per document); default 32768 */
  normalizeMaxBytes?: number
  /** garbage collection of the normalized snapshot and of the responder's / fan-out's replies: 'document' (default) follows
   *  each live document's own `gc` option (yDocOptions), true / false force it.  A custom gcFilter cannot be reproduced:
   *  use normalize: false with one. */
  gc?: 'document' | boolean
}

export declare class GpuMerge implements Extension {
  extensionName: string
  priority: number
  constructor (configuration?: GpuMergeConfiguration)
  onConfigure (): Promise<void>
  onLoadDocument (data: onLoadDocumentPayload): Promise<void>
  afterLoadDocument (data: afterLoadDocumentPayload): Promise<void>
  onChange (data: onChangePayload): Promise<void>
  onStoreDocument (data: onStoreDocumentPayload): Promise<void>
  afterUnloadDocument (data: afterUnloadDocumentPayload): Promise<void>
  onDestroy (): Promise<void>
  /** one version (yjs's encoded snapshot) per loaded document, one GPU batch; unloaded or refused documents are left out */
  takeVersions (names: string[]): Promise<Map<string, Uint8Array>>
  /** the documents as they were at the versions (Y.createDocFromSnapshot), one GPU batch, one settled result per entry;
   *  a gc: true document's entry is rejected with "originDoc must not be garbage collected" */
  restoreVersions (entries: { documentName: string, version: Uint8Array, gc?: boolean }[]): Promise<({ status: 'fulfilled', value: Uint8Array } | { status: 'rejected', reason: Error })[]>
  /** what each loaded document says (field 'default', deep true by default), one GPU batch; unloaded or refused documents are left out */
  textOf (names: string[], opts?: { field?: string, deep?: boolean }): Promise<Map<string, string>>
  /** restoreVersions followed by one text batch over the fulfilled results, settled per entry */
  versionTexts (entries: { documentName: string, version: Uint8Array, gc?: boolean }[], opts?: { field?: string, deep?: boolean }): Promise<({ status: 'fulfilled', value: string } | { status: 'rejected', reason: Error })[]>
  /** what each loaded document is: JSON.stringify(TiptapTransformer.fromYdoc(document, field)) (field 'default'), or the
   *  parsed object with parse: true, one GPU batch; unloaded documents are left out, refused ones left out and named in `unserialized`.
   *  field: a root name; null or [] for every field (fromYdoc(document), the webhook body); string[] for those fields --
   *  the last two give the object keyed by field */
  jsonOf (names: string[], opts?: { field?: string | FieldList, parse?: boolean }): Promise<Map<string, string | object>>
  /** restoreVersions followed by one JSON batch over the fulfilled results, settled per entry; field as jsonOf's */
  versionJson (entries: { documentName: string, version: Uint8Array, gc?: boolean }[], opts?: { field?: string | FieldList, parse?: boolean }): Promise<({ status: 'fulfilled', value: string | object } | { status: 'rejected', reason: Error })[]>
  /** what each loaded document's Map / Array / Text root is, in one GPU batch: JSON.stringify(document.getMap(root).toJSON())
   *  (type 'map', the default), getArray ('array') or getText ('text'), or the parsed value with parse: true; unloaded
   *  documents are left out, refused ones left out and named in `unserialized`. */
  sharedJsonOf (names: string[], opts?: { root?: string, type?: 'map' | 'array' | 'text', parse?: boolean }): Promise<Map<string, string | object>>
  /** restoreVersions followed by one toJSON batch over the fulfilled results, settled per entry; root, type as sharedJsonOf's */
  versionSharedJson (entries: { documentName: string, version: Uint8Array, gc?: boolean }[], opts?: { root?: string, type?: 'map' | 'array' | 'text', parse?: boolean }): Promise<({ status: 'fulfilled', value: string | object } | { status: 'rejected', reason: Error })[]>
  /** documents whose JSON the engine refused in jsonOf / versionJson / sharedJsonOf / versionSharedJson: the caller keeps its yjs path (transformer.fromYdoc) for them */
  unserialized: { documentName: string, code: string }[]
  /** batched SyncStep1 responder over the captured state (snapshot + updates since) */
  syncResponder (): SyncResponder
  /** batched extension-redis fan-out over the same captured state */
  redisFanout (opts: { publish: (channel: string, message: Buffer) => any, identifier?: string, prefix?: string, windowMs?: number, onError?: (e: Error) => void }): RedisFanout
}
