'use strict'
// Version history through the extension: node test/version.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs (Y.snapshot / Y.createDocFromSnapshot per call);
//          checks what the extension asks of the engine
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), byte for byte against yjs
// Two live gc: false documents get versions between edits, text is deleted, the documents are stored and reloaded, and
// restoreVersions brings the deleted text back -- the bytes of yjs's own createDocFromSnapshot path; a gc: true
// document's entry is rejected without disturbing the others.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const Y = require(path.join(__dirname, '..', '..', '..', 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle

const hex = b => Buffer.from(b).toString('hex')
const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))

// test double (never shipped): the engine calls the extension makes, from yjs; the two version ops are the new ones
class VersionDouble {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { this.log.push(['mergeMany', docs.length]); return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { this.log.push(['takeVersionMany', states.length]); return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) {
    this.log.push(['restoreVersionMany', states.length, opts ? Array.from(opts, isNoGc) : null])
    return states.map((s, i) => {
      try { return yjsRestore(s, versions[i], !(opts && isNoGc(opts[i]))) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) }
    })
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine () {
  if (mode === 'cpu') return new VersionDouble()
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
}

const tests = []
const test = (name, fn) => tests.push({ name, fn })

test('versions of two live gc: false documents restore deleted text after a store and a reload', async () => {
  const engine = makeEngine()
  const store = new MemoryStore()
  const ext = new GpuMerge({ engine, store, Y })
  try {
    const a = await openDoc(ext, 'a', false, 21)
    const b = await openDoc(ext, 'b', false, 22)
    const c = await openDoc(ext, 'c', true, 23)
    a.document.getText('t').insert(0, 'the quick brown fox 😀 jumps')
    b.document.getMap('m').set('k', 'first'); b.document.getText('t').insert(0, 'second document')
    c.document.getText('t').insert(0, 'collected')
    const v1 = await ext.takeVersions(['a', 'b', 'c', 'nobody'])
    assert.deepStrictEqual(Array.from(v1.keys()).sort(), ['a', 'b', 'c'])
    for (const [n, d] of [['a', a.document], ['b', b.document], ['c', c.document]]) assert.strictEqual(hex(v1.get(n)), hex(Y.encodeSnapshot(Y.snapshot(d))), n)
    const textA = a.document.getText('t').toString()
    // more edits, a second version, then the deletions
    a.document.getText('t').insert(4, 'very ')
    b.document.getMap('m').set('k', 'second')
    const v2 = await ext.takeVersions(['a', 'b'])
    assert.strictEqual(hex(v2.get('a')), hex(Y.encodeSnapshot(Y.snapshot(a.document))))
    const textA2 = a.document.getText('t').toString()
    a.document.getText('t').delete(2, 22)   // (through the surrogate pair)
    b.document.getText('t').delete(0, 7)
    c.document.getText('t').delete(0, 3)
    await Promise.all([ext.onStoreDocument(a), ext.onStoreDocument(b), ext.onStoreDocument(c)])
    for (const p of [a, b, c]) await ext.afterUnloadDocument(p)
    const a2 = await openDoc(ext, 'a', false, 31)
    const b2 = await openDoc(ext, 'b', false, 32)
    const c2 = await openDoc(ext, 'c', true, 33)
    assert.strictEqual(a2.document.getText('t').toString(), a.document.getText('t').toString())
    a2.document.getText('t').insert(0, 'after the reload: ')   // (base and log: merged before the batch)

    const stateA = Y.encodeStateAsUpdate(a2.document); const stateB = Y.encodeStateAsUpdate(b2.document)
    const res = await ext.restoreVersions([
      { documentName: 'a', version: v1.get('a') }, { documentName: 'c', version: v1.get('c') },
      { documentName: 'b', version: v1.get('b'), gc: false }, { documentName: 'a', version: v2.get('a'), gc: false },
      { documentName: 'nobody', version: v1.get('a') }, { documentName: 'b', version: v2.get('b') }])
    assert.deepStrictEqual(res.map(r => r.status), ['fulfilled', 'rejected', 'fulfilled', 'fulfilled', 'rejected', 'fulfilled'])
    assert.strictEqual(res[1].reason.message, 'originDoc must not be garbage collected')
    assert.throws(() => Y.createDocFromSnapshot(c2.document, Y.decodeSnapshot(v1.get('c'))), /originDoc must not be garbage collected/)
    assert.strictEqual(hex(res[0].value), hex(yjsRestore(stateA, v1.get('a'), true)))
    assert.strictEqual(hex(res[2].value), hex(yjsRestore(stateB, v1.get('b'), false)))
    assert.strictEqual(hex(res[3].value), hex(yjsRestore(stateA, v2.get('a'), false)))
    assert.strictEqual(hex(res[5].value), hex(yjsRestore(stateB, v2.get('b'), true)))
    // the user-visible point: the deleted text is back
    assert.strictEqual(load(res[0].value, true).getText('t').toString(), textA)
    assert.strictEqual(load(res[3].value, false).getText('t').toString(), textA2)
    assert.strictEqual(load(res[2].value, false).getMap('m').get('k'), 'first')
    assert.strictEqual(load(res[2].value, false).getText('t').toString(), 'second document')
    assert.strictEqual(load(res[5].value, true).getMap('m').get('k'), 'second')
    if (mode === 'cpu') {
      const calls = engine.log.filter(x => x[0] === 'restoreVersionMany')
      assert.deepStrictEqual(calls, [['restoreVersionMany', 4, [false, true, true, false]]])   // one batch, the rejected entries never sent
      assert.deepStrictEqual(engine.log.filter(x => x[0] === 'takeVersionMany'), [['takeVersionMany', 3], ['takeVersionMany', 2]])
    }

    // a per-document refusal (a version ahead of the state) rejects that entry alone
    const ahead = Y.encodeSnapshot(Y.createSnapshot(Y.createDeleteSet(), new Map([[31, 1000]])))
    const mixed = await ext.restoreVersions([{ documentName: 'a', version: ahead }, { documentName: 'b', version: v1.get('b') }])
    assert.strictEqual(mixed[0].status, 'rejected'); assert.strictEqual(mixed[0].reason.code, 'EINVAL')
    assert.strictEqual(hex(mixed[1].value), hex(yjsRestore(stateB, v1.get('b'), true)))
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test('the addon: calls of one window share a batch; explicit batches; a bad option byte fails its document only', async () => {
    const engine = makeEngine()
    try {
      const d = new Y.Doc({ gc: false }); d.clientID = 9
      d.getText('t').insert(0, 'hello brave new world')
      const v = Y.encodeSnapshot(Y.snapshot(d))
      d.getText('t').delete(3, 12)
      const u = Y.encodeStateAsUpdate(d)
      const s0 = engine.stats()
      const [x, y] = await Promise.all([engine.restoreVersion(u, v), engine.restoreVersion(u, v, { gc: false })])
      assert.strictEqual(engine.stats().docsSnapshot - s0.docsSnapshot, 4, 'one restore batch of two documents')
      assert.strictEqual(hex(x), hex(yjsRestore(u, v, true)))
      assert.strictEqual(hex(y), hex(yjsRestore(u, v, false)))
      const [t1, t2] = await Promise.all([engine.takeVersion(u), engine.takeVersion(Y.encodeStateAsUpdate(new Y.Doc()))])
      assert.strictEqual(hex(t1), hex(Y.encodeSnapshot(Y.snapshot(d))))
      assert.strictEqual(hex(t2), '0000')
      const many = await engine.restoreVersionMany([u, u, u], [v, v, v], [0, 2, { gc: false }])
      assert.strictEqual(hex(many[0]), hex(x)); assert.strictEqual(hex(many[2]), hex(y))
      assert.ok(many[1] instanceof Error && many[1].code === 'EINVAL')
      assert.deepStrictEqual((await engine.takeVersionMany([u, u])).map(hex), [hex(t1), hex(t1)])
    } finally { engine.close() }
  })
}

;(async () => {
  let failed = 0
  for (const t of tests) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : tests.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
